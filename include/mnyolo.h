/* libmnyolo — C ABI of the MI355X-native MobileNet-YOLO hot path (gfx950 only).
 *
 * Drop-in boundary B2 of SURVEY §8(b).  The reference (eric612/Mobilenet-YOLO-Pytorch)
 * owns no kernels: its hot path is stock torch.nn ops + torchvision.ops.nms.  Each entry
 * point below therefore cites the reference CALL SITE whose arithmetic it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *  - Activations are channels-last (NHWC) fp32 unless stated otherwise.
 *  - "View" arguments (x, in_scale, in_shift, in_act): the kernel reads
 *        a = act(x * in_scale[c] + in_shift[c])      (in_scale == NULL -> a = act(x))
 *    i.e. the BatchNorm-apply + activation of the PRODUCING layer is fused into the
 *    consumer's load path; padding taps are 0 in the activated domain.
 *  - `stats` (optional, may be NULL): per-channel partial sums of the raw output,
 *    laid out [parts][2][C] (sum, sum of squares); `parts` is returned by the matching
 *    *_stat_parts() query.  mny_bn_finalize() reduces them in fp64.
 *  - Ownership: the caller allocates every buffer (inputs, outputs, workspaces).  The
 *    library never allocates, frees or retains device pointers.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*); no entry point
 *    synchronises the device.
 *  - Return value: 0 on success, a negative MNY_E* code otherwise; mny_last_error()
 *    returns a thread-local message.  No C++ exception crosses this boundary.
 *  - Re-entrant; deterministic (no floating-point atomics anywhere).
 */
#ifndef MNYOLO_H
#define MNYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden visibility: these declarations are all it exports */
#pragma GCC visibility push(default)

#define MNY_OK 0
#define MNY_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define MNY_EHIP (-2)     /* a HIP runtime call / kernel launch failed */
#define MNY_EUNSUPPORTED (-3)

/* activation codes (mobilenetv2.py:42 ReLU6, mbv2_yolo.py:24 LeakyReLU(0.1),
 * mobilenetv3.py:14-23 hswish / ReLU) */
#define MNY_ACT_NONE 0
#define MNY_ACT_RELU6 1
#define MNY_ACT_LEAKY 2
#define MNY_ACT_RELU 3
#define MNY_ACT_HSWISH 4
#define MNY_ACT_HSIGMOID 5   /* relu6(z+3)/6, mobilenetv3.py:20-23; only as the gate operand of mny_mul_views */

int mny_version(void);
const char* mny_last_error(void);
/* max number of stat/partial rows any kernel will write (upper bound for workspace sizing) */
int mny_max_parts(void);

/* ---- stem: 3x3 stride-2 pad-1 conv 3->Cout on NCHW input, NHWC output -------------------
 * replaces nn.Conv2d(3,32,3,2,1) at models/mobilenetv2.py:40 (used :113).               */
int mny_stem_fwd(const float* x_nchw, const float* w /*[Cout,3,3,3]*/, float* y /*[N,H/2,W/2,Cout]*/,
                 float* stats, int N, int H, int W, int Cout, void* stream);
int mny_stem_stat_parts(int N, int H, int W, int Cout);
/* dW = sum x * dy; `ws` holds [mny_stem_wgrad_parts()][Cout*27] floats */
int mny_stem_wgrad(const float* x_nchw, const float* dy, float* dw, float* ws,
                   int N, int H, int W, int Cout, void* stream);
int mny_stem_wgrad_parts(int N, int H, int W, int Cout);

/* weight gradient of the stem conv straight from the stem unit's OUTPUT gradient g (what autograd hands to
 * BatchNorm's backward, mobilenetv2.py:40-42): dY = ca*g*act'(scale*y+shift) + cb*y + cc is rebuilt on load from
 * g and the raw conv output y (coef = mny_bn_bwd_finalize's [3][Cout]), so mny_bn_bwd_apply's dY tensor is
 * neither written nor re-read.  ws as for mny_stem_wgrad.  Cout with 256 % (Cout/4) == 0. */
int mny_stem_bnwgrad_supported(int Cout);
int mny_stem_bnwgrad(const float* x_nchw, const float* g, const float* y, const float* scale,
                     const float* shift, int act, const float* coef, float* dw, float* ws, int N, int H, int W,
                     int Cout, void* stream);

/* ---- depthwise KxK (K=3|5), stride 1|2, pad K/2, no bias ---------------------------------
 * replaces nn.Conv2d(C,C,3,s,1,groups=C) at models/mobilenetv2.py:65,79 and
 * models/mbv2_yolo.py:22 (BasicConv depthwise); K=5 for models/mobilenetv3.py:54.        */
int mny_dw_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act,
               const float* w /*[C,K,K]*/, float* y, float* stats,
               int N, int H, int W, int C, int K, int stride, void* stream);
int mny_dw_stat_parts(int N, int H, int W, int C, int K, int stride);
/* the same count for a given storage type: flags bit 0 = bf16 storage.  On bf16 storage the 5x5 stride-1 launches with >= 120 channels (last
 * 64-channel chunk at least 3/4 full) run the TILE form of csrc/dwtile.hip (every thread loads and activates its own column once, the
 * window comes back from an LDS ring; MNY_DWTF=0 / 1 forces never / always), which has its own grid. */
int mny_dw_stat_parts_x(int N, int H, int W, int C, int K, int stride, int flags);
/* dx[N,H,W,C] = (addend ? addend : 0) + conv_transpose(dy, w); H,W are the INPUT extents */
int mny_dw_bwd_data(const float* dy, const float* w, const float* addend, float* dx,
                    int N, int H, int W, int C, int K, int stride, void* stream);
/* dw[C,K,K]; ws holds [mny_dw_wgrad_parts()][C*K*K] floats */
int mny_dw_bwd_weight(const float* x, const float* in_scale, const float* in_shift, int in_act,
                      const float* dy, float* dw, float* ws,
                      int N, int H, int W, int C, int K, int stride, void* stream);
int mny_dw_wgrad_parts(int N, int H, int W, int C, int K, int stride);

/* ---- pointwise 1x1 conv == row-major GEMM on fp32 MFMA ----------------------------------
 * y[M,Nc] = act_in(x)[M,K] * w[Nc,K]^T (+ bias) (+ addend)
 * replaces nn.Conv2d(Cin,Cout,1) at models/mobilenetv2.py:48,69,75,83,
 * models/mbv2_yolo.py:20 (BasicConv 1x1) and :82 (biased head conv).
 * The same entry point computes the data gradient: dx[M,K] = dy[M,Nc] * wT[K,Nc]^T with
 * wT = mny_transpose(w) and `addend` = the other gradient contribution (residual path). */
int mny_pw_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act,
               const float* w, const float* bias, const float* addend, float* y, float* stats,
               int64_t M, int K, int Nc, void* stream);
int mny_pw_stat_parts(int64_t M, int K, int Nc);
/* dw[Nc,K] = dy[M,Nc]^T * act_in(x)[M,K]; dbias[Nc] (optional) = column sums of dy.
 * ws holds mny_pw_wgrad_ws_floats() floats (the same query serves mny_pw_wgrad_bf16: it covers the partial rows of
 * either storage type, so at a 96-wide side, where the bf16 plan has up to twice the splits, the fp32 caller's workspace is sized for the bf16 plan too). */
int mny_pw_wgrad(const float* x, const float* in_scale, const float* in_shift, int in_act,
                 const float* dy, float* dw, float* dbias, float* ws,
                 int64_t M, int K, int Nc, void* stream);
size_t mny_pw_wgrad_ws_floats(int64_t M, int K, int Nc);
/* Fused BatchNorm-backward + weight gradient + data gradient of a pointwise unit whose input has <= 32 channels
 * (the HBM-bound "expand" layers of models/mobilenetv2.py:75-77, e.g. 16->96 @176x176): replaces
 * mny_bn_bwd_reduce/finalize/apply + mny_pw_wgrad + mny_transpose + mny_pw_fwd(dgrad) and never materialises dY
 * (DESIGN.md §4).  g = dL/d act(scale*y+shift); x is read through its view; dx (optional) = data gradient wrt the
 * activated input (+ addend).  ws: mny_pw_bnbwd_ws_floats() floats.  mny_pw_bnbwd_supported() tells whether a shape qualifies. */
int mny_pw_bnbwd_supported(int64_t M, int K, int Nc);
size_t mny_pw_bnbwd_ws_floats(int64_t M, int K, int Nc);
int mny_pw_bnbwd(const float* g, const float* y, const float* scale, const float* shift, int act,
                 const float* mean, const float* invstd, const float* gamma,
                 const float* x, const float* in_scale, const float* in_shift, int in_act,
                 const float* w, const float* addend, float* dx, float* dw, float* dgamma, float* dbeta,
                 float* ws, int64_t M, int K, int Nc, void* stream);
/* mny_pw_bnbwd whose data gradient completes the output gradient of the conv+BN+act unit in front of the expand unit (the project conv of the previous
 * block, directly or through the residual add that hands it the gradient unchanged): that unit's BN-backward sums (sum dz, sum dz*xhat over the STORED dx;
 * ry = its raw output [M][K], r_scale / r_shift / r_act = its view, clamp family) leave with the second stage, red[mny_pw_bnbwd_red_parts()][2][K] —
 * no mny_bn_bwd_reduce pass over (dx, ry).  fp32 storage, N in {96, 144, 192} (mny_pw_bnbwd_red_supported). */
int mny_pw_bnbwd_red_supported(int64_t M, int K, int Nc);
int mny_pw_bnbwd_red_parts(int64_t M, int K, int Nc);
int mny_pw_bnbwd_red(const float* g, const float* y, const float* scale, const float* shift, int act, const float* mean, const float* invstd,
                     const float* gamma, const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                     const float* addend, float* dx, float* dw, float* dgamma, float* dbeta, float* ws, const float* ry, const float* r_scale,
                     const float* r_shift, int r_act, const float* r_mean, const float* r_invstd, float* red, int64_t M, int K, int Nc, void* stream);
int mny_transpose(const float* src /*[R,Cc]*/, float* dst /*[Cc,R]*/, int R, int Cc, void* stream);

/* ---- BatchNorm (training / eval), eps 1e-5, momentum 0.1 ---------------------------------
 * replaces nn.BatchNorm2d at models/mobilenetv2.py:41,49,66,70,76,80,84 and
 * models/mbv2_yolo.py:23.  Training: stats partials -> batch mean/var (biased for the
 * normalisation, unbiased for running_var like torch) -> scale/shift consumed by views. */
int mny_bn_finalize(const float* stats, int parts, int64_t count,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var,   /* updated in place; may be NULL */
                    float* scale, float* shift, float* mean, float* invstd, int C, void* stream);
int mny_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift,
                       int C, void* stream);
/* backward, step 1: partial sums of dz = g * act'(scale*y+shift) and dz*yhat,
 * yhat = (y-mean)*invstd  -> red[parts][2][C] */
int mny_bn_bwd_reduce(const float* g, const float* y, const float* scale, const float* shift, int act,
                      const float* mean, const float* invstd, float* red, int64_t M, int C, void* stream);
int mny_bn_bwd_parts(int64_t M, int C);
/* step 2: dgamma, dbeta and the per-channel coefficients of dy = ca*dz + cb*y + cc */
int mny_bn_bwd_finalize(const float* red, int parts, int64_t count, const float* gamma,
                        const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* coef /*[3][C]*/, int C, void* stream);
/* step 3: dy = ca * g*act'(scale*y+shift) + cb*y + cc   (dy may alias g).
 * coef == NULL: dy = g*act'(...) only (activation backward of a non-BN view). */
int mny_bn_bwd_apply(const float* g, const float* y, const float* scale, const float* shift, int act,
                     const float* coef, float* dy, int64_t M, int C, void* stream);

/* ---- residual / upsample glue -----------------------------------------------------------
 * out = view(a) + view(b) [+ nearest-2x-upsample(up)]   (all [N,H,W,C]; up is [N,H/2,W/2,C])
 * replaces `x + self.conv(x)` (mobilenetv2.py:89), torch.add (mbv2_yolo.py:103,151) and
 * nn.Upsample(scale_factor=2,'nearest') (mbv2_yolo.py:52).  b may be NULL (materialise a). */
int mny_add_views(const float* a, const float* a_scale, const float* a_shift, int a_act,
                  const float* b, const float* b_scale, const float* b_shift, int b_act,
                  const float* up, float* out, int N, int H, int W, int C, void* stream);
/* out = view(a) * view(b): the per-pixel "SE" gate of models/mobilenetv3.py:40-41 (x * hsigmoid(bn(conv(..)))).
 * backward of one operand: dst = (addend ? addend : 0) + g * view(other). */
int mny_mul_views(const float* a, const float* a_scale, const float* a_shift, int a_act,
                  const float* b, const float* b_scale, const float* b_shift, int b_act,
                  float* out, int64_t M, int C, void* stream);
int mny_mul_views_bwd(const float* g, const float* o, const float* o_scale, const float* o_shift, int o_act,
                      const float* addend, float* dst, int64_t M, int C, void* stream);
/* PartAdd(a, upsample2x(up)) of models/mbv3_yolo.py:85-96,135 for Ca <= Cb:
 * out[..., :Ca] = view(a) + up2x[..., :Ca];  out[..., Ca:] = up2x[..., Ca:].   out/up2x have Cb channels. */
int mny_partadd_up(const float* a, const float* a_scale, const float* a_shift, int a_act, const float* up,
                   float* out, int N, int H, int W, int Ca, int Cb, void* stream);
/* dst[M,Ca] = (accumulate ? dst : 0) + src[M,Cb][:, :Ca]   (gradient of the PartAdd's first operand) */
int mny_slice_channels(const float* src, float* dst, int accumulate, int64_t M, int Ca, int Cb, void* stream);
/* dst[N,H/2,W/2,C] = (accumulate ? dst : 0) + sum of the 2x2 children of src[N,H,W,C] */
int mny_upsample_bwd(const float* src, float* dst, int accumulate, int N, int H, int W, int C, void* stream);
/* dst = (accumulate ? dst : 0) + alpha[0] * src   (alpha: device scalar or NULL => 1) */
int mny_axpy(const float* src, const float* alpha, float* dst, int accumulate, int64_t n, void* stream);

/* ---- detection math ---------------------------------------------------------------------
 * One head, channels-last [N,g,g,A*(5+C)] (channel = a*(5+C)+attr, yolo_loss.py:84).
 * anchors_all: [n_anchors_all][2] already divided by img_size (yolo_loss.py:214);
 * mask: the A indices of this head's anchors.
 * targets: packed [T,5] = (label 1..C, cx, cy, w, h); t_off[N+1] = per-image offsets.  */
typedef struct {
    int N, g, A, C;            /* batch, grid, anchors of this head, classes */
    int n_anchors_all;
    float ignore_thresh, iou_thresh, iou_weighting;
} mny_yolo_head;

/* Training: replaces YOLOLoss.forward/get_target (models/yolo_loss.py:77-178,206-236),
 * box_ciou (:257-293), class_loss (:425-434), weighted_mse_loss (:53-60) and their autograd
 * graph.  out7 = (loss, recall, avg_iou, obj, no_obj, cls_score, count/N); dhead = dLoss/dhead.
 * ws: mny_yolo_loss_ws_bytes() bytes. */
int mny_yolo_loss(const float* head, const float* targets, const int32_t* t_off,
                  const float* anchors_all, const int32_t* mask, const mny_yolo_head* hp,
                  float* out7, float* dhead, void* ws, void* stream);
size_t mny_yolo_loss_ws_bytes(const mny_yolo_head* hp, int total_targets);

/* Eval: replaces YOLOLoss.get_pred_boxes (models/yolo_loss.py:180-204): decode every cell to
 * (x1,y1,x2,y2,conf,cls_score,cls_idx), keep conf > val_conf, compact per image preserving
 * (anchor,row,col) order.  Image n writes rows[n*row_stride + base + i]; base = base_counts[n]
 * (NULL -> 0) so a second head can append behind the first (utils/box.py:17 `cat`);
 * counts[n] = base + kept.  row_stride >= A*g*g (+ what earlier heads may have written). */
int mny_yolo_decode(const float* head, const float* anchors_all, const int32_t* mask,
                    const mny_yolo_head* hp, float val_conf, float* rows, int row_stride,
                    const int32_t* base_counts, int32_t* counts, void* stream);

/* Per-class NMS: replaces utils/box.py:11-31 + torchvision.ops.nms(boxes, score*conf, thr).
 * rows: [capacity,7]; segment s (one image) = rows[seg_begin[s] .. seg_begin[s]+seg_count[s]).
 * out_idx: kept row indices (into rows); segment s occupies out_idx[seg_begin[s] ..
 * +out_counts[s]), class-major then descending score (stable, ties by original order).
 * out_rows (optional): the kept rows gathered densely, segment after segment.
 * thr is a double and the float IoU is promoted before the strict `>` compare, like torchvision.
 * max_seg_rows: caller's upper bound on rows in any one segment (sizes the LDS sort buffer;
 * 0 = use `capacity`).  No bucket-size limit (utils/box.py:20-29 has none): a (segment,class)
 * bucket beyond the 8192-row LDS image is sorted and resolved through global scratch.  Only a
 * WRONG bound (a real segment larger than max_seg_rows) is an error: such a bucket keeps nothing
 * and the int32 at ws+mny_nms_status_offset() receives its size (0 = ok).
 * The int32[S+1] exclusive prefix of out_counts is left at ws+mny_nms_prefix_offset().
 * ws: mny_nms_ws_bytes() bytes. */
int mny_nms_per_class(const float* rows, const int32_t* seg_begin, const int32_t* seg_count, int S,
                      int capacity, int max_seg_rows, int num_classes, double thr,
                      int32_t* out_idx, int32_t* out_counts, float* out_rows, void* ws, void* stream);
size_t mny_nms_ws_bytes(int S, int capacity, int num_classes);
size_t mny_nms_status_offset(int S, int capacity, int num_classes);
size_t mny_nms_prefix_offset(int S, int capacity, int num_classes);

/* ---- test-time augmentation of the detection path (csrc/tta.hip; Ultralytics' `--augment` and merge-NMS) ----
 * The batch goes through the network as several views (sizes, some mirrored); every view's decoded candidates
 * are appended, un-mirrored, into one segment per image, ONE per-class NMS runs over the union, and optionally
 * every kept box is replaced by the score-weighted mean of the candidates of its class that overlap it.  The
 * rows are normalised (mny_yolo_decode), so a change of scale needs no box arithmetic.  No host sync, no
 * atomics, results bit-reproducible; tests/tta_ref.py restates the three stages in numpy.
 *
 * mny_tta_view: src[N,C,Hs,Ws] fp32 NCHW -> dst[N,C,Hd,Wd]: mirror, then bilinear resize with half-pixel
 *   centres and no antialiasing (F.interpolate(mode="bilinear", align_corners=False) semantics), in fp64:
 *     sy = max((y + 0.5) * ((double)Hs / Hd) - 0.5, 0);  y0 = (int)sy;  y1 = min(y0 + 1, Hs - 1);  ly = sy - y0
 *     (the same for x with Ws, Wd: sx, x0, x1, lx);  with `flip` source column c is read from Ws - 1 - c;
 *     a, b = src[y0][x0], src[y0][x1];  c, d = src[y1][x0], src[y1][x1], promoted to double;
 *     dst[y][x] = (float)((1-ly) * ((1-lx)*a + lx*b) + ly * ((1-lx)*c + lx*d)): every product and sum one fp64
 *     operation (no contraction), one rounding at the end.  A term whose weight is exactly 0 is skipped, not
 *     multiplied, at both levels (a sum with one term left is that term's product): a non-finite neighbour
 *     cannot poison an exact sample, and Hd == Hs, Wd == Ws is an exact (mirrored) copy.
 *   Any sizes >= 1 are legal (the multiple-of-32 rule belongs to the network); src != dst.
 *
 * mny_det_append: rows are [.,7] as mny_yolo_decode writes them.  For image n:
 *   copied = max(0, min(src_counts[n], src_stride, dst_stride - counts[n])) (0 when counts[n] is outside
 *   0..dst_stride); rows src_rows[n*src_stride + r], r < copied, are written in source order to
 *   dst_rows[n*dst_stride + counts[n] + r]; then counts[n] += copied.  With `flip` the written row has
 *   x1' = 1.0f - x2 and x2' = 1.0f - x1 (one fp32 subtraction each); columns 1, 3 and 4..6 are copied.
 *   The clamp keeps every write inside the image's segment; a caller that sizes dst_stride as the sum of its
 *   sources' strides never meets it.  One workgroup per image.  N == 0 is valid.
 *
 * mny_nms_merge: runs after mny_nms_per_class (with out_rows) over the same rows and segments; out_prefix is
 *   the int32[S+1] prefix that call leaves at ws + mny_nms_prefix_offset().  For segment s and
 *   r < out_counts[s]: i = out_idx[seg_begin[s] + r] is a kept row, c = rows[i][6] its class, and its output
 *   row is out_rows[out_prefix[s] + r].  Members: the rows j of segment s with rows[j][6] == c and
 *   (j == i or (double)iou(i, j) > thr), where iou is the fp32 arithmetic of the NMS (kept box i first):
 *     area = (x2 - x1) * (y2 - y1);  xx1 = i.x1 > j.x1 ? i.x1 : j.x1, yy1 likewise;
 *     xx2 = i.x2 < j.x2 ? i.x2 : j.x2, yy2 likewise;  w = xx2 - xx1, h = yy2 - yy1, each set to 0 unless > 0
 *     (negative or NaN);  inter = w * h;  iou = inter / (area_i + area_j - inter).
 *   Weight w_j = rows[j][5] * rows[j][4] (one fp32 product, the NMS score).  In ascending j, in fp64:
 *   sw += w_j;  sx_k += (double)w_j * (double)rows[j][k], k = 0..3 (the products are exact).  Then
 *   out_rows[.][k] = (float)(sx_k / sw), or rows[i][k] when sw is not finite and positive.  Columns 4..6 and
 *   the order of out_rows are untouched.  The summation order is part of the specification.
 *   Design bound: segments of up to a few thousand rows — one lane per kept box walks its whole segment
 *   (staged through LDS in chunks of 256 rows), time O(kept x rows) per segment on at most 8 workgroups;
 *   larger segments are correct, only slow.  S == 0, empty segments and out_counts == 0 are valid. */
int mny_tta_view(const float* src, float* dst, int N, int C, int Hs, int Ws, int Hd, int Wd, int flip,
                 void* stream);
int mny_det_append(const float* src_rows, int src_stride, const int32_t* src_counts, int flip,
                   float* dst_rows, int dst_stride, int32_t* counts, int N, void* stream);
int mny_nms_merge(const float* rows, const int32_t* seg_begin, const int32_t* seg_count, int S,
                  const int32_t* out_idx, const int32_t* out_counts, const int32_t* out_prefix, double thr,
                  float* out_rows, void* stream);

/* ---- post-processing options of the detection path (csrc/postproc.hip; Ultralytics' non_max_suppression protocol) ----
 * Opt-in: mny_yolo_decode / mny_nms_per_class are what they were.  A score threshold, a candidate per (cell, class)
 * pair (`multi_label`), a class filter, class-agnostic NMS and a cap on the detections per image (`max_det`).  The
 * row format (x1, y1, x2, y2, conf, cls, class) is unchanged, so the NMS, mny_nms_merge and the evaluators read the
 * rows as before.  No host sync, no atomics, results bit-reproducible; tests/post_ref.py restates the three stages.
 *
 * mny_yolo_decode_ex: head, anchors_all, mask, hp, rows, row_stride, base_counts and counts as mny_yolo_decode.
 *   For image n and every cell in (anchor, gy, gx) order, with the arithmetic of mny_yolo_decode (one definition,
 *   csrc/detshare.h): box = the decoded corners, conf = sigmoid(t4), cls_c = sigmoid(t[5+c]) with
 *   sigmoid(x) = 1.0f / (1.0f + expf(-x)); b = the first c with the largest cls_c (a NaN never wins; b = 0 when no
 *   cls_c exceeds -inf).  score_c = conf * cls_c, one fp32 product: the product the NMS forms from columns 4 and 5.
 *     allowed(c) = class_mask == NULL or bit (c & 31) of class_mask[c >> 5] is set   (DEVICE uint32 words)
 *     pass(c)    = conf > obj_thr and (score_thr < 0 or score_c > score_thr) and allowed(c)
 *   All compares are strict and a NaN fails them; a negative score_thr switches the score test off.
 *   multi_label == 0: the cell emits (box, conf, cls_b, b) when pass(b).
 *   multi_label != 0: the cell emits (box, conf, cls_c, c) for every c with pass(c), c ascending.
 *   Candidates are numbered t = 0, 1, ... in that order (cells, then classes).  base = base_counts[n] (NULL -> 0);
 *   room = row_stride - base when 0 <= base <= row_stride, else 0.  Candidate t is written to
 *   rows[n*row_stride + base + t] when t < room, and to nowhere otherwise: nothing is written outside the image's
 *   segment.  counts[n] = base + min(total, room);  dropped[n] = total - min(total, room)  (DEVICE int32 [N]).
 *   row_stride >= 1 is the only requirement; the caller checks `dropped` with the counts.  With multi_label = 0,
 *   score_thr < 0, class_mask = NULL and row_stride >= A*g*g the rows and counts are mny_yolo_decode's bit for bit.
 *
 * mny_nms_agnostic: the result of mny_nms_per_class on the same rows with column 6 read as 0 and num_classes = 1
 *   (one bucket per segment: descending score = rows[i][5] * rows[i][4], ties by original order; the same kernels,
 *   a segment beyond the 8192-row LDS image goes through global scratch).  out_idx, out_counts, the prefix and the
 *   status word are as there, under the offsets of mny_nms_agnostic_*_offset(); out_rows carries the ORIGINAL rows,
 *   class included.  ws: mny_nms_agnostic_ws_bytes() bytes.
 *
 * mny_det_topk: runs after either NMS (same rows, seg_begin, capacity) and before mny_nms_merge; in place on
 *   out_idx / out_counts / out_rows.  For segment s: k = out_counts[s] clamped to 0 .. capacity - seg_begin[s];
 *   entry r < k is the row i_r = out_idx[seg_begin[s] + r] with score_r = rows[i_r][5] * rows[i_r][4] (one fp32
 *   product; 0 when i_r is not in 0 .. capacity-1).  Order the entries by the NMS's own key, ascending:
 *     u = bits of score_r;  u = (u & 0x80000000) ? ~u : (u | 0x80000000);  key = (~u << 32) | r
 *   i.e. descending score, ties by position in the NMS output, -0 behind +0, a NaN with the sign bit clear ahead of
 *   +inf and one with it set behind -inf, as inside an NMS bucket.  kept = min(k, max_det): the first `kept` entries'
 *   row indices are written to out_idx[seg_begin[s] + 0 .. kept-1], out_counts[s] = kept, out_prefix (int32 [S+1],
 *   caller's buffer) = the exclusive prefix of the new counts, and out_rows (optional) is regathered densely from
 *   `rows`, segment after segment.  k <= max_det only reorders.  max_det <= 0 is an argument error; S == 0 and empty
 *   segments are valid.  mny_nms_merge then works on the reduced lists without change (pass it out_prefix).
 *   ws: mny_det_topk_ws_bytes() bytes.  One workgroup per segment; more than 4096 kept entries in one segment are
 *   sorted through global scratch (correct, slow). */
int mny_yolo_decode_ex(const float* head, const float* anchors_all, const int32_t* mask,
                       const mny_yolo_head* hp, float obj_thr, float score_thr, int multi_label,
                       const uint32_t* class_mask, float* rows, int row_stride,
                       const int32_t* base_counts, int32_t* counts, int32_t* dropped, void* stream);
int mny_nms_agnostic(const float* rows, const int32_t* seg_begin, const int32_t* seg_count, int S,
                     int capacity, int max_seg_rows, double thr, int32_t* out_idx, int32_t* out_counts,
                     float* out_rows, void* ws, void* stream);
size_t mny_nms_agnostic_ws_bytes(int S, int capacity);
size_t mny_nms_agnostic_status_offset(int S, int capacity);
size_t mny_nms_agnostic_prefix_offset(int S, int capacity);
int mny_det_topk(const float* rows, const int32_t* seg_begin, int S, int capacity, int max_det,
                 int32_t* out_idx, int32_t* out_counts, float* out_rows, int32_t* out_prefix, void* ws,
                 void* stream);
size_t mny_det_topk_ws_bytes(int S, int capacity);

/* ---- sliced (tiled) inference of the detection path (csrc/slice.hip; SAHI's get_sliced_prediction) ----
 * The ORIGINAL image is cut into overlapping tiles at native resolution, every tile goes through the network as an
 * image of its own, its candidates are mapped back into the original image and appended to that image's segment
 * (optionally with the candidates of one whole-image view, for the large objects), and ONE NMS runs over the union.
 * Opt-in: mny_prep_batch and mny_det_append are what they were.  No host sync, no atomics on row positions, results
 * bit-reproducible; tests/slice_ref.py restates the three stages in numpy.
 *
 * The tile grid (host, slicing.tile_grid(h, w, tile_h, tile_w, overlap_h, overlap_w); the rule is SAHI's get_slice_bboxes):
 *   the ratios lie in [0, 1);  oy = (int)(overlap_h * tile_h), ox = (int)(overlap_w * tile_w), both below the tile's size
 *   (anything else is an argument error).  Rows k = 0, 1, ...: start = k * (tile_h - oy), end = start + tile_h; row k is
 *   (y0, y1) = (start, end) when end <= h and is shifted back to (max(0, h - tile_h), h) when end would pass h; row 0 always
 *   exists and row k + 1 exists when row k's unshifted end lies below h.  Columns the same with w, tile_w, ox.  Windows
 *   (x0, y0, x1, y1) in integer pixels, row-major.  Every tile of an image that is at least tile-sized has the tile's size; an
 *   image smaller than the tile in one axis gives windows clamped to the image in that axis.  Duplicate windows are not removed.
 *   1280 x 720, tile 416, overlap 0.2: x starts 0, 333, 666, 864 and y starts 0, 304.
 *
 * mny_prep_tiles: slot b of out [B,3,out_h,out_w] is what mny_prep_batch writes for a dense copy of the window
 *   src + tiles[b].offset, h x w pixels, rows `pitch` bytes apart: Pillow's im.crop(box).resize((out_w, out_h), BILINEAR), then
 *   ToTensor and Normalize, bit for bit.  The window is an image of its own: the tap tables are those of an h x w image, so
 *   the taps at the window's edge clamp at the window and never read the neighbouring pixels of the source image
 *   (Image.resize(box=) reads them and is not the model).  A window of the output's size is a copy plus the normalisation (the
 *   coefficient rule gives a single unit tap).  Windows of different slots may overlap.
 *   image == -1: a padding slot, written as zeros, no status.  A window outside 1..max_h x 1..max_w or with pitch < 3*w
 *   is written as zeros and the int32 at ws+0 receives 1 + b (0 = ok), as in mny_prep_batch.  The caller keeps
 *   offset + (h-1)*pitch + 3*w inside src.  tiles: DEVICE [B].  mean3/std3: HOST.  ws: mny_prep_tiles_ws_bytes().
 *
 * mny_det_append_tiles: rows are [.,7] as mny_yolo_decode writes them, slot b's at src_rows + b*src_stride*7, normalised to
 *   the slot's window.  The result is that of processing the slots b = 0..B-1 in ascending order.  Slot b with
 *   n = maps[b].image in 0..N-1 (any other value, -1 = padding: nothing is appended):
 *     read the rows r < min(src_counts[b], src_stride) (none when that is <= 0), in source order;
 *     drop a row (x1, y1, x2, y2, ...) when, with every compare strict in fp32 (a NaN coordinate is kept),
 *       (interior & 1) && x1 < ex   or   (interior & 4) && x2 > 1.0f - ex   or
 *       (interior & 2) && y1 < ey   or   (interior & 8) && y2 > 1.0f - ey
 *     (the cut-object rule: a box that touches an interior tile edge belongs to an object that a neighbouring, overlapping
 *     tile sees whole; a side of the window on the image border is never tested);
 *     a surviving row is written with columns 0 and 2 = (float)(ax + bx * (double)v) and columns 1 and 3 =
 *     (float)(ay + by * (double)v): one fp64 product, one fp64 sum (no contraction), one rounding; columns 4..6 are copied;
 *     nothing is clipped to [0, 1] (mny_yolo_decode does not clip either).  ax = 0, bx = 1, interior = 0: bit-identical copies
 *     (of every value but -0.0, which the sum turns into +0.0).
 *     The survivors are numbered t = 0, 1, ... in source order;  room = dst_stride - counts[n] when
 *     0 <= counts[n] <= dst_stride, else 0 (the rule of mny_det_append);  survivor t is written to
 *     dst_rows[n*dst_stride + counts[n] + t] when t < room and to nowhere otherwise: nothing is written outside the image's
 *     segment.  Then counts[n] += min(total, room) and dropped[n] += total - min(total, room)  (DEVICE int32 [N]; the
 *     caller zeroes `dropped` and checks it with the counts).
 *   The order is part of the specification (the NMS breaks score ties by row order).  One workgroup per image walks the
 *   slots; within a slot the compaction is an ordered wave scan, as in mny_yolo_decode_ex.  maps: DEVICE [B].
 *   B == 0 and N == 0 are valid. */
typedef struct mny_tile_desc {
    int64_t offset; /* bytes from src to the window's pixel (0,0) */
    int32_t h, w;   /* window size in pixels */
    int32_t pitch;  /* bytes between source rows (>= 3*w) */
    int32_t image;  /* destination image of the slot's candidates; -1 = padding slot */
} mny_tile_desc;
typedef struct mny_tile_map {
    double ax, bx, ay, by; /* x' = ax + bx * x : ax = x0 / W, bx = (x1 - x0) / W, formed on the host in double; y likewise */
    float ex, ey;          /* edge margins in tile-normalised units: (float)(edge / out_w), (float)(edge / out_h) */
    int32_t image;         /* destination image, -1 = padding slot (nothing appended) */
    uint32_t interior;     /* bit 0 left, 1 top, 2 right, 3 bottom: that side of the window is NOT on the image border */
} mny_tile_map;
size_t mny_prep_tiles_ws_bytes(int B, int max_h, int max_w, int out_h, int out_w);
int mny_prep_tiles(const uint8_t* src, const mny_tile_desc* tiles, int B, int max_h, int max_w, int out_h, int out_w,
                   const float* mean3, const float* std3, float* out, void* ws, void* stream);
int mny_det_append_tiles(const float* src_rows, int src_stride, const int32_t* src_counts, const mny_tile_map* maps, int B,
                         float* dst_rows, int dst_stride, int32_t* counts, int32_t* dropped, int N, void* stream);

/* ---- fused backward of a depthwise 3x3 stride-1 conv + BN + activation unit ----------------------------
 * One pass over (g, y, x) instead of bn_bwd_apply + dw_bwd_weight + dw_bwd_data (7 tensor passes -> 4): rebuilds
 * dY = ca*g*act'(scale*y+shift) + cb*y + cc in registers from the coefficients `coef` = [3][C] written by
 * mny_bn_bwd_finalize, and produces dx (gradient wrt the ACTIVATED input view, + optional addend) and dw [C,1,3,3].
 * `ws`: [mny_dw_bnbwd_parts_k()][C*K*K] floats.  K == 3 or K == 5, stride == 1 (mny_dw_bnbwd_supported()).
 * replaces the backward of mobilenetv2.py:65-67,79-81 / mbv2_yolo.py:22-24 for those units.
 * K == 5 (MobileNetV3's 5x5 units, mobilenetv3.py:54-56,68-69) runs the TILE form (csrc/dwtile.hip): a workgroup owns a tile of
 * columns x channel groups, dY is rebuilt once per element and shared through a ring of K+1 rows in LDS, every window element
 * feeds the data gradient (gather) and the weight gradient (over the input pixels a thread owns); dw is [C,1,5,5].  On bf16 storage
 * the 3x3 units the tile form is faster on take it too (dwt_use() in dwtile.hip states the rule and the measurements).
 * MNY_NO_DWT5=1 reports K == 5 unsupported (bn_bwd_apply + dw_bwd_weight + dw_bwd_data); MNY_DWT3=1 / 0 forces 3x3 onto / off the tile form.
 * mny_dw_bnbwd_parts_k(..., flags): bit 0 = bf16 storage, bit 1 = called as mny_dw_bnbwd_red (the row count depends on the form that runs);
 * mny_dw_bnbwd_parts() == mny_dw_bnbwd_parts_k(..., 3, 0). */
int mny_dw_bnbwd_supported(int K, int stride);
int mny_dw_bnbwd_parts(int N, int H, int W, int C);
int mny_dw_bnbwd_parts_k(int N, int H, int W, int C, int K, int flags);
int mny_dw_bnbwd(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                 const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                 const float* addend, float* dx, float* dw, float* ws, int N, int H, int W, int C, int K, int stride,
                 void* stream);
/* The same fusion for a 3x3 STRIDE-2 depthwise unit (x is [N,H,W,C], g / y are [N,Ho,Wo,C] with Ho = (H-1)/2+1): replaces
 * mny_bn_bwd_apply + mny_dw_bwd_weight + mny_dw_bwd_data of the four down-sampling units (models/mobilenetv2.py:65-67 at
 * stride 2).  ws: [mny_dw_bnbwd_s2_parts()][C*9] floats; dw == NULL leaves the partials to mny_reduce_batch. */
int mny_dw_bnbwd_s2_parts(int N, int H, int W, int C);
int mny_dw_bnbwd_s2(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                    const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                    const float* addend, float* dx, float* dw, float* ws, int N, int H, int W, int C, void* stream);
/* mny_dw_bnbwd + the BN-backward sums of the unit that PRODUCED the input: when `x` is the raw output of a conv+BN+act unit
 * (in_scale/in_shift/in_act = its view, in_mean/in_invstd = its batch statistics) whose only consumer is this depthwise unit,
 * the dX written here is that unit's complete output gradient, and the kernel also leaves its sums (sum dz, sum dz*xhat per
 * channel) as partial rows in_red[mny_dw_bnbwd_parts()][2][C] — the input of mny_bn_bwd_finalize that a separate
 * mny_bn_bwd_reduce pass over (dX, x) would have produced (autograd of BatchNorm2d + ReLU6 at models/mobilenetv2.py:69-71). */
int mny_dw_bnbwd_red(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                     const float* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                     const float* in_invstd, const float* w, const float* addend, float* dx, float* dw, float* ws, float* in_red,
                     int N, int H, int W, int C, int K, int stride, void* stream);

/* ---- low-rank BatchNorm backward of a WIDE expand unit (csrc/lrbwd.hip) --------------------------------------------------------
 * autograd of nn.Conv2d(K, C, 1) + nn.BatchNorm2d + ReLU6 / ReLU / h-swish with C >= 2K (models/mobilenetv2.py:73-78,
 * models/mobilenetv3.py:49-51,67) WITHOUT the bn_bwd_apply pass over the C-wide tensors.  The depthwise unit behind it stores
 * dzc = ca o dL/da o act'(z) (ca = gamma * invstd = the unit's forward scale) instead of dL/da (mny_dw_bnbwd_red_dz: same arguments and
 * partial rows as mny_dw_bnbwd_red); then with X the unit's viewed K-wide input and Y = X W^T:
 *     dX = dzc W + X Q + r,    Q = W^T diag(cb) W,  r = cc^T W          (mny_pw_fwd data gradient on dzc, then mny_pw_lr_fix)
 *     dW = dzc^T X + cb o (W G) + cc (x) s,   G = X^T X,  s = colsum(X)   (mny_pw_wgrad on dzc, then mny_lr_wfix)
 * with (ca, cb, cc) = the coefficient rows of mny_bn_bwd_finalize.
 * mny_lr_gram : partial rows [mny_lr_gram_parts(M, K)][K*K + K] = (G | s) of the VIEWED input (combine with mny_reduce_batch).
 * mny_lr_prep : q[K][K] = Q (symmetric, so it is its own NT operand) and r[K], on the fp32 matrix cores.
 * mny_pw_lr_fix : dx = view(x) Q + r + addend (addend may be dx; in_scale / in_shift = the LINEAR view of the unit's input, or NULL, NULL);
 *               red != NULL: the BN-backward sums of the unit whose complete output gradient dx now is (ry = its raw output [M][K], r_* = its
 *               view / statistics), rows [mny_pw_lr_fix_parts(M, K, r_act)][2][K].
 * mny_lr_wfix : dw[C][K] += cb o (W G) + cc (x) s in place; gram_sums = the combined [K*K + K] row of mny_lr_gram.               */
int mny_lr_supported(int64_t M, int K, int C);
int mny_lr_gram_parts(int64_t M, int K);
int mny_lr_gram(const float* x, const float* in_scale, const float* in_shift, int in_act, float* parts, int64_t M, int K, void* stream);
int mny_lr_gram_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, float* parts, int64_t M, int K, void* stream);
int mny_lr_prep(const float* coef, const float* w, float* q, float* r, int C, int K, void* stream);
int mny_pw_lr_fix_parts(int64_t M, int K, int r_act);
int mny_pw_lr_fix(const float* x, const float* in_scale, const float* in_shift, const float* q, const float* r, const float* addend, float* dx,
                  const float* ry, const float* r_scale, const float* r_shift, int r_act, const float* r_mean, const float* r_invstd, float* red,
                  int64_t M, int K, void* stream);
int mny_lr_wfix(float* dw, const float* gram_sums, const float* coef, const float* w, int C, int K, void* stream);
/* ... and for a 3x3 STRIDE-2 unit (fp32 storage, ReLU6 view of the producer): mny_dw_bnbwd_s2 with dx = in_scale o dX o relu6'(z) and the producer's
 * BN-backward sums as partial rows in_red[mny_dw_bnbwd_s2_parts()][2][C] (models/mobilenetv2.py:73-81 at stride 2: block 96 -> 576 -> 160). */
int mny_dw_bnbwd_s2_red_dz(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                           const float* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                           const float* in_invstd, const float* w, const float* addend, float* dx, float* dw, float* ws, float* in_red,
                           int N, int H, int W, int C, void* stream);
/* Fused backward of a depthwise 5x5 STRIDE-2 conv+BN+act unit (models/mobilenetv3.py:88,100: Block(5, 24->72->40, s2), Block(5, 160->672->160, s2);
 * replaces the autograd backward of nn.Conv2d(groups=C, 5, stride 2, pad 2) + nn.BatchNorm2d + ReLU / h-swish): dY rebuilt from (g, y, coef) on
 * chip, one pass over (g, y, x) yields dx (+ addend) and the weight-gradient partials ws[mny_dw_bnbwd_s2k5_parts()][C*25] (dw == NULL leaves them to
 * mny_reduce_batch).  in_red != NULL (with in_mean / in_invstd / in_scale / in_shift of the unit that produced x, consumed only here): that unit's
 * BN-backward sums as partial rows in_red[parts][2][C].  C even. */
int mny_dw_bnbwd_s2k5_parts(int N, int H, int W, int C);
int mny_dw_bnbwd_s2k5(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                      const float* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                      const float* in_invstd, const float* w, const float* addend, float* dx, float* dw, float* ws, float* in_red,
                      int N, int H, int W, int C, void* stream);
int mny_dw_bnbwd_s2k5_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* coef,
                           const void* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                           const float* in_invstd, const float* w, const void* addend, void* dx, float* dw, float* ws, float* in_red,
                           int N, int H, int W, int C, void* stream);
int mny_dw_bnbwd_red_dz_supported(int K, int C, int bf16);
int mny_dw_bnbwd_red_dz(const float* g, const float* y, const float* scale, const float* shift, int act, const float* coef,
                        const float* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                        const float* in_invstd, const float* w, const float* addend, float* dx, float* dw, float* ws, float* in_red,
                        int N, int H, int W, int C, int K, int stride, void* stream);

/* ---- row padding for the detection heads' backward ---------------------------------------------------------
 * The head gradient dL/dhead is [M][75] (yolo_loss.py:84 channel layout): rows are neither 16-B aligned nor a multiple
 * of 4 wide, which would put its weight- and data-gradient GEMMs on the register-staged kernels.  mny_pad_rows copies it
 * (times *alpha, the upstream dL/dloss; alpha may be NULL) into [M][Cp] with zeroed pad columns, mny_transpose_pad
 * writes W^T as [Cin][Cp] with zeroed pad columns; the GEMMs then run with Cp channels (pad products are 0, the pad rows
 * of dW land in the slack of the caller's gradient slot).                                                      */
int mny_pad_rows(const float* src, const float* alpha, float* dst, int64_t M, int C, int Cp, void* stream);
int mny_transpose_pad(const float* src /*[R][Cc]*/, float* dst /*[Cc][Rp]*/, int R, int Cc, int Rp, void* stream);

/* ---- all weight transposes of a backward pass in one launch ----------------------------------------------------
 * The data-gradient GEMMs read W^T ([Cin][Cout] rows; mny_transpose / mny_transpose_pad per layer).  A static plan
 * knows every (W, W^T) pair up front: jobs (DEVICE array) describe them, block_job (DEVICE int32[nblocks]) maps a
 * 32x32-tile workgroup to its job (job.block0 = its first workgroup; a job has ceil(Cc/32)*ceil(Rp/32) of them). */
/* Deferred partial combines.  Every weight-gradient entry point (mny_pw_wgrad, mny_dw_bwd_weight, mny_dw_bnbwd[_red],
 * mny_stem_wgrad, mny_stem_bnwgrad and their _bf16 twins) writes per-workgroup partial sums [nparts][n] to `ws` and then
 * combines them (fp64, fixed order) into dW.  Called with dw == NULL it stops after the partials (mny_pw_wgrad: only without
 * dbias); a static plan gives each layer its own `ws` and combines a whole backward segment in ONE launch: jobs (DEVICE
 * array) name the partials, block_job (DEVICE int32[nblocks]) maps a workgroup (32 outputs) to its job (job.block0 = its first
 * workgroup, ceil(n/32) of them).  Same arithmetic and order as the per-layer combine. */
typedef struct mny_reduce_job {
    const float* parts; /* [nparts][n] */
    float* out;         /* [n] */
    int64_t n;
    int32_t nparts, block0;
} mny_reduce_job;
int mny_reduce_batch(const mny_reduce_job* jobs, const int32_t* block_job, int nblocks, void* stream);
int mny_pw_wgrad_splits(int64_t M, int K, int Nc);      /* nparts of mny_pw_wgrad's partials (n = Nc * K) */

typedef struct mny_transpose_job {
    const float* src; /* [R][Cc] fp32 */
    void* dst;        /* [Cc][Rp] fp32 (or bf16 for the _bf16 entry point), columns R..Rp-1 zeroed */
    int32_t R, Cc, Rp, block0;
} mny_transpose_job;
int mny_transpose_batch(const mny_transpose_job* jobs, const int32_t* block_job, int nblocks, void* stream);

/* ---- fused multi-tensor AdamW --------------------------------------------------------------
 * replaces optim.AdamW(...).step() at train.py:134,283 (torch semantics: decoupled weight decay, bias-corrected
 * moments, amsgrad off).  `table_dev` is a DEVICE array of chunks; one workgroup updates one chunk (callers split
 * large tensors into chunks of <= 64 Ki elements).  `vec4` = all four pointers 16-B aligned.  `step` is the
 * 1-based step count used for the bias corrections.                                                            */
typedef struct mny_adamw_chunk {
    float* p;
    const float* g;
    float* m;
    float* v;
    int n;
    int vec4;
} mny_adamw_chunk;
int mny_adamw_step(const mny_adamw_chunk* table_dev, int nchunks, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, void* stream);

/* ---- fused multi-tensor SGD, weight EMA and shadow swap (no reference counterpart beyond train.py:457's --momentum) --
 * The same DEVICE chunk table and launch shape as mny_adamw_step (one workgroup per chunk of the caller's length, float4
 * body, scalar tail); each entry point reads only the fields listed, and `vec4` means "every pointer THIS entry point
 * uses is 16-B aligned".  Scalars are derived in double and rounded to float once.  No float atomics: deterministic.
 *
 * mny_sgd_step — torch.optim.SGD(maximize=False).step().  Reads p, g, n, vec4, and m when momentum != 0 (m may be
 *   NULL otherwise: it is neither read nor written); v is unused.  Per element
 *       d = g + weight_decay * p                                      (skipped exactly when weight_decay == 0)
 *       momentum != 0:  buf = d when `first`, else momentum * buf + (1 - dampening) * d       (buf = m, written back)
 *                       d = nesterov ? d + momentum * buf : buf
 *       p -= lr * d
 *   `first` = these chunks have no momentum buffer yet (torch's `momentum_buffer is None`): m is only written.
 * mny_ema_update — m <- m + (1 - decay) * (p - m), torch.lerp's form for a weight below 0.5 (one fmaf).  Reads p
 *   (read only), m, n, vec4; g and v are unused.
 * mny_swap_chunks — exchanges p[0..n) and m[0..n) exactly; two calls are the identity bit for bit.  Reads p, m, n,
 *   vec4; g and v are unused.
 * MNY_EINVAL (before any launch): null table or nchunks <= 0; negative (or NaN) lr, momentum, weight_decay; nesterov
 * with momentum <= 0 or dampening != 0 (torch's ValueError); decay outside [0, 1] (NaN included).                 */
int mny_sgd_step(const mny_adamw_chunk* table_dev, int nchunks, double lr, double momentum, double dampening,
                 double weight_decay, int nesterov, int first, void* stream);
int mny_ema_update(const mny_adamw_chunk* table_dev, int nchunks, double decay, void* stream);
int mny_swap_chunks(const mny_adamw_chunk* table_dev, int nchunks, void* stream);

/* ---- fused gradient clipping (torch.nn.utils.clip_grad_norm_, L2, in two launches) ----------------------------
 * `segs_dev` is a DEVICE array of gradient segments: g[0..n) fp32, 4-byte aligned, any n >= 0.  A segment of n floats
 * is cut into mny_grad_clip_parts(n) blocks of MNY_CLIP_BLOCK floats; `block0` is the number of blocks of the
 * segments in front of it (non-decreasing, 0 for the first) and `nblocks` their total.  Nothing outside
 * [g, g + n) is read or written, so slack between segments never enters the norm.
 * Launch 1: one workgroup per block leaves the block's sum of squares in ws[block] (double): a fixed partition
 * summed in a fixed order — a thread's fp32 accumulator takes at most MNY_CLIP_TERMS squares, everything across
 * threads and blocks is fp64 — so two runs agree bit for bit.  Launch 2: every workgroup combines ws[] the same
 * way, out[0] = total_norm = (float)sqrt(sum), out[1] = coef = min(1, max_norm / (total_norm + 1e-6)) with one
 * correctly rounded fp32 division (torch multiplies max_norm by the rounded reciprocal, which can differ in the last bit; out[1] is the
 * factor that was applied).  A non-finite norm propagates as it does in torch: NaN stays NaN.  g *= coef in place unless coef == 1.
 * `ws`: nblocks doubles; `out`: 2 floats; both device memory.  No host synchronisation.                        */
#define MNY_CLIP_BLOCK 8192
#define MNY_CLIP_TERMS 34 /* 8 float4 of the 16-byte aligned body + one scalar each of its head and tail */
typedef struct mny_clip_seg {
    float* g;
    int64_t n;
    int32_t block0;
    int32_t pad;
} mny_clip_seg;
int mny_grad_clip_parts(int64_t n);
int mny_grad_clip(const mny_clip_seg* segs_dev, int nsegs, int nblocks, double max_norm, double* ws, float* out, void* stream);

/* ---- data-gradient GEMM + BN-backward reduction of the unit it feeds ------------------------------------------
 * dx[M,Nc] = dy[M,K] * W, with W^T given as [Nc][K] rows (mny_transpose of the conv weight) — the autograd
 * data gradient of nn.Conv2d(Nc,K,1) (mobilenetv2.py:69,83) — when dx is the complete gradient of a
 * conv+BN+act unit's output: the epilogue also forms that unit's BN-backward sums from the tile it just
 * produced and the unit's raw output y[M,Nc]:  red[part][0][c] = sum dz, red[part][1][c] = sum dz*xhat,
 * dz = dx * act'(scale*y+shift), xhat = (y-mean)*invstd — exactly what mny_bn_bwd_reduce(dx, y, ...) writes,
 * in the same [parts][2][Nc] layout (parts = mny_pw_dgrad_bnred_parts(M,K,Nc)); feed it to mny_bn_bwd_finalize.
 * Saves the reduce pass's read of dx.  K % 4 == 0 (K % 8 for the bf16 twin), any activation. */
int mny_pw_dgrad_bnred_supported(int64_t M, int K, int Nc, int act);
int mny_pw_dgrad_bnred_parts(int64_t M, int K, int Nc); /* partial rows it writes */
int mny_pw_dgrad_bnred(const float* dy, const float* wT, float* dx, const float* y, const float* scale,
                       const float* shift, int act, const float* mean, const float* invstd, float* red,
                       int64_t M, int K, int Nc, void* stream);
/* ... with an addend: dx = dy * W + addend is the LAST contribution to that unit's output gradient (the others — a residual
 * branch — were accumulated into `addend`), and the sums are taken over the complete dx (torch.add at mobilenetv2.py:89 followed
 * by the BatchNorm backward of the block's project conv). */
int mny_pw_dgrad_bnred_add_supported(int64_t M, int K, int Nc, int act);
int mny_pw_dgrad_bnred_add(const float* dy, const float* wT, const float* addend, float* dx, const float* y, const float* scale,
                           const float* shift, int act, const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc,
                           void* stream);

/* ---- fp32 GEMMs on pre-cut weight planes ---------------------------------------------------------------------------
 * The MFMA-bound fp32 GEMMs run on the bf16 matrix cores as six partial products per fp32 product (every operand cut exactly into
 * three bf16 pieces).  The weight operand is the same for every row tile: a static plan cuts all of its GEMM weights
 * (and their transposes) ONCE per pass with mny_cut3_batch — jobs (DEVICE array) name fp32 matrices [R][C] and their plane buffers of
 * mny_pw_w6_bytes(C, R) bytes, block_job (DEVICE int32[nblocks]) maps a workgroup (256 16-byte chunks) to its job (job.block0 = its
 * first workgroup, ceil(R * ceil(C/16) * 2 / 256) of them) — and calls the _w6 twins, which take the planes where mny_pw_fwd /
 * mny_pw_dgrad_bnred[_add] take the fp32 matrix.  Same tiling, same partial rows (mny_pw_stat_parts / mny_pw_dgrad_bnred_parts), same
 * results up to fp32 rounding order.  mny_pw_w6_supported(M, K, Nc): the shape takes this form (fp32, K % 4 == 0, >= 20 FLOP per byte). */
typedef struct mny_cut3_job {
    const float* src; /* [R][C] fp32 */
    void* dst;        /* three bf16 planes, mny_pw_w6_bytes(C, R) bytes */
    int32_t R, C, block0, pad;
} mny_cut3_job;
int mny_pw_w6_supported(int64_t M, int K, int Nc);
size_t mny_pw_w6_bytes(int K, int Nc);
int mny_cut3_batch(const mny_cut3_job* jobs, const int32_t* block_job, int nblocks, void* stream);
int mny_pw_fwd_w6(const float* x, const float* in_scale, const float* in_shift, int in_act, const void* w6, const float* bias,
                  const float* addend, float* y, float* stats, int64_t M, int K, int Nc, void* stream);
int mny_pw_dgrad_bnred_w6(const float* dy, const void* wT6, const float* addend, float* dx, const float* y, const float* scale,
                          const float* shift, int act, const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc,
                          void* stream);

/* ---- which kernel family a pointwise-conv call takes (pure host query; tests and tools/plan_stats.py use it to PROVE that a
 * plan compared with the oracle contains the kernels the benchmark runs) ----------------------------------------------------------
 * op: 0 = mny_pw_fwd (forward / plain data gradient of nn.Conv2d(K,Nc,1), mobilenetv2.py:63-85), 1 = mny_pw_dgrad_bnred[_add],
 * 2 = mny_pw_wgrad (no bias gradient).  bf16: the storage type of the plan (0 = fp32).  Returns one of MNY_ROUTE_*: the launchers' own
 * rule (the function every *_parts / *_splits / *_supported query asks as well) evaluated for a call with a plain view — no input
 * view, bias, addend or bias gradient.  After such a call mny_pw_last_route returns the same value; a call behind an h-swish view or
 * with a bias (gradient) can take another family. */
enum {
    MNY_ROUTE_TILE_V1 = 0,      /* register-staged tile kernels (unaligned channel counts) */
    MNY_ROUTE_DMA_F32 = 1,      /* LDS-DMA tile kernel, fp32 MFMA (or the bf16 MFMA with bf16 storage) */
    MNY_ROUTE_DMA_X6 = 2,       /* LDS-DMA tile kernel, six-product bf16 form */
    MNY_ROUTE_THIN = 3,         /* short-reduction vector-ALU stream kernel (pwthin.hip) */
    MNY_ROUTE_WIDE = 4,         /* barrier-free wide-output kernel (pwwide.hip) */
    MNY_ROUTE_WGRAD_STREAM = 5, /* barrier-free stream weight-gradient kernel (pwwgs.hip) */
    MNY_ROUTE_WAVE16 = 6        /* bf16 storage, K <= 48 at >= 131072 pixels: a wave per 16 pixels on the bf16 matrix cores (gate.hip pwt_fwd_kernel) */
};
int mny_pw_route(int op, int bf16, int64_t M, int K, int Nc);   /* the family of a plain-view call (no h-swish input, no bias gradient) */
/* the family the LAST pointwise-conv call of the calling thread actually took (every launcher records the route it acted on; -1 before
 * the first call).  engine.py records it for every call of a plan's first replay: NetPlan.kernel_routes() reports what ran. */
int mny_pw_last_route(void);
/* Which KERNEL a weight-gradient call launches (pure host query), from the decision the launcher itself acts on:
 * template * 1000 + MODE * 100 + TI * 10 + TJ, template 0 = register-staged pw_wgrad_kernel, 1 = LDS-DMA fp32 MFMA, 2 = LDS-DMA six-product
 * form, 3 = LDS-DMA bf16 storage, 5 = the stream kernel (tile digits 0).  has_view: in_scale / in_shift are passed; bias_grad: dbias is.
 * The six-product form exists for five MODE 0 tiles; a call of the MNY_ROUTE_DMA_X6 family on any other tile (every MODE 1 plan, e.g.
 * K 96 N 576) launches the fp32-MFMA kernel of that tile and reports template 1 here while its family stays MNY_ROUTE_DMA_X6.
 * MNY_EINVAL on an empty problem.  mny_pw_wgrad_last_kernel: the code of the calling thread's last mny_pw_wgrad[_bf16] call (-1 before). */
int mny_pw_wgrad_kernel(int bf16, int64_t M, int K, int Nc, int in_act, int has_view, int bias_grad);
int mny_pw_wgrad_last_kernel(void);

/* ---- evaluation consumer: VOC07 11-point mAP on the device -----------------------------
 * Replaces utils/eval_mAP.py:134-187 (calculate_mAP), :69-132 (eval_class_ap), :8-65
 * (eval_single_image_recall) and utils/iou.py:4-48 (find_jaccard_overlap) on a PACKED layout: the
 * reference's per-image tensor lists laid back to back, image i = [off[i], off[i+1]).
 * n_classes counts the background entry (train.py:58); classes 1..n_classes-1 are evaluated, labels are
 * float like the reference's tensors (a label that is not an integer in that range is never evaluated).
 * Semantics kept: within an image detections are matched in STORED order; best ground truth = first
 * maximum of the fp32 IoU (NaN -> false positive); IoU > 0.5; a hit on a `difficult` (true_diff != 0)
 * object counts as neither; a second hit on an object is a false positive.  Score ties in the global sort
 * keep (image, stored) order (torch.sort leaves them unspecified).
 * Outputs (device): ap[n_classes-1], tp_sum / fp_sum [n_classes-1] (exact counts as float),
 * prec11 [(n_classes-1)*11] (the 11 interpolated precisions), mean_ap[1].
 * Limits: n_classes <= 255, D <= 2^30.  ws: mny_map_ws_bytes(D, T) bytes.  No host sync. */
size_t mny_map_ws_bytes(int64_t D, int64_t T);
int mny_map_eval(const float* det_boxes /*[D,4]*/, const float* det_labels, const float* det_scores,
                 const int32_t* det_off /*[n_images+1]*/, const float* true_boxes /*[T,4]*/,
                 const float* true_labels, const float* true_diff, const int32_t* true_off, int n_images,
                 int64_t D, int64_t T, int n_classes, float* ap, float* tp_sum, float* fp_sum, float* prec11,
                 float* mean_ap, void* ws, void* stream);
/* train.py:371-385 (the glue of test() between the detector and calculate_mAP): detection rows
 * [D,7] (x1,y1,x2,y2,obj,cls_conf,cls) -> boxes, label = cls+1, score = obj*cls_conf; targets [T,5]
 * (cls,cx,cy,w,h) -> corner boxes, label = cls as stored, difficulty 0.  Either half may be empty. */
int mny_eval_pack(const float* rows, int64_t D, const float* targets, int64_t T, float* det_boxes,
                  float* det_labels, float* det_scores, float* true_boxes, float* true_labels,
                  float* true_diff, void* stream);

/* ---- COCO-style detection metrics on the device (csrc/cocoeval.hip) ------------------------------------
 * AP averaged over IoU thresholds, AP by object size, AR at detection caps: the arithmetic of
 * pycocotools.cocoeval.COCOeval for iouType='bbox' on the packed layout of mny_map_eval.  The package is not
 * available where this library is developed, so the entry is NOT pinned against it: the rules below (restated
 * in numpy, float64, in tests/coco_ref.py) are the specification.
 * Inputs: as mny_map_eval with true_crowd[T] (!= 0: crowd) in place of true_diff; image_sizes[n_images,2] =
 * (w, h) in pixels, NULL = (1, 1).  Classes 1..n_classes-1; a label that is not an integer in that range is
 * never evaluated.  Parameters are HOST arrays, copied into the launch: iou_thrs[n_iou <= 16],
 * rec_thrs[n_rec <= 128], max_dets[n_maxdet <= 4] (positive, ascending), area_rngs[n_area <= 8][2] (lo, hi in
 * pixels^2), stat_desc[S <= 32][4] = (is_recall, IoU index or -1 = all, area index, cap index).
 * Geometry (fp64, no fused multiply-add): X1 = x1*W, Y1 = y1*H, X2 = x2*W, Y2 = y2*H, w = X2-X1, h = Y2-Y1,
 *   area = w*h; iw = min(dX1+dw, gX1+gw) - max(dX1, gX1), IoU 0 if iw <= 0, ih alike; inter = iw*ih;
 *   union = crowd(g) ? area(d) : (area(d) + area(g)) - inter; iou = inter / union.
 * Per (image, class) with a detection: detections sorted by descending score (stable in stored order,
 *   -0.0 == 0.0, NaN last) and cut to max_dets[-1].
 * Per area range: a ground truth is ignored if it is a crowd or its area is < lo or > hi; ground truths are
 *   visited not-ignored first, then ignored, each group in stored order.
 * Per threshold t, each detection in score order: best = min(t, 1-1e-10), m = none; for each ground truth:
 *   skip it if matched at this t and no crowd; stop if m is not ignored and this one is; skip it if
 *   iou < best; else best = iou, m = this (among equal IoUs the later one wins).  A matched detection inherits
 *   m's ignore flag and marks m matched; an unmatched one whose own area is outside the range is ignored.
 * Accumulate per (class k, area a, cap c): the first max_dets[c] detections of every (image, class) list,
 *   in image order, sorted by descending score (stable); npig = not-ignored ground truths of (k, a); with
 *   npig == 0 the entries are -1.  Per threshold: tp = cumsum(matched & ~ignored), fp = cumsum(~matched &
 *   ~ignored), rc = tp/npig, pr = tp/(fp+tp+2.220446049250313e-16); recall = rc[-1] (0 without detections);
 *   pr becomes its running maximum from the right; precision[r] = pr[first i with rc[i] >= rec_thrs[r]], 0
 *   if there is none.
 * Outputs (device, fp64): precision[n_iou,n_rec,K,n_area,n_maxdet], recall[n_iou,K,n_area,n_maxdet] with
 *   K = n_classes-1; stats[S]: the mean of the entries > -1 of the slice a stat_desc row names (precision
 *   over recall thresholds and classes, or recall over classes), -1 if there are none; per_class_ap[K]: the
 *   same over all thresholds at area range 0 and the last cap.  Optional (NULL to skip), in STORED detection
 *   order: det_match[n_area,n_iou,D] = packed index of the matched ground truth, -1 unmatched, -2 not
 *   evaluated (rank >= max_dets[-1] or label out of range); det_ignore[n_area,n_iou,D] = 0 / 1.
 * Counts are exact and precision / recall are single fp64 divisions of them; the means are fixed-order sums.
 * No host sync, no floating-point atomics, deterministic.  Limits: n_classes <= 255, n_images < 2^24,
 * D, T <= 2^30, and the parameter counts above; beyond them MNY_EINVAL (mny_coco_ws_bytes returns 0) with a
 * mny_last_error text.  The number of ground truths per (image, class) has no limit.
 * ws: mny_coco_ws_bytes(...) bytes. */
size_t mny_coco_ws_bytes(int64_t D, int64_t T, int n_images, int n_classes, int n_iou, int n_rec, int n_area,
                         int n_maxdet);
int mny_coco_eval(const float* det_boxes /*[D,4]*/, const float* det_labels, const float* det_scores,
                  const int32_t* det_off /*[n_images+1]*/, const float* true_boxes /*[T,4]*/,
                  const float* true_labels, const float* true_crowd, const int32_t* true_off,
                  const float* image_sizes /*[n_images,2], NULL = (1,1)*/, int n_images, int64_t D, int64_t T,
                  int n_classes, const double* iou_thrs, int n_iou, const double* rec_thrs, int n_rec,
                  const int32_t* max_dets, int n_maxdet, const double* area_rngs, int n_area,
                  const int32_t* stat_desc /*[S,4]*/, int S, double* precision, double* recall, double* stats,
                  double* per_class_ap, int32_t* det_match, uint8_t* det_ignore, void* ws, void* stream);

/* ---- validation report on the device (csrc/detreport.hip) ----------------------------------------------
 * Precision / recall / F1 of every class over a grid of confidences, the confidence that maximises the
 * smoothed mean F1, and a detection confusion matrix.  Nothing in the reference computes them and no third-
 * party package is pinned: the rules below (restated in numpy, float64, in tests/report_ref.py) are the
 * specification.  The curves are exact step functions of the detection set { score >= c }; the np.interp of
 * other trainers' curves is not reproduced.  All fp64 arithmetic is done as separate IEEE operations in the
 * order written (the file is compiled with -ffp-contract=off); integer counts are exact.
 *
 * mny_det_curves.  Inputs (device): det_labels[D], det_scores[D]; det_match[D] (int32: >= 0 matched, -1
 *   unmatched, -2 not evaluated) and det_ignore[D] (uint8), one [area, iou] slice of mny_coco_eval's optional
 *   outputs; true_labels[T], true_crowd[T].  K = n_classes-1 classes (n_classes counts the background entry,
 *   2..255), a grid of G points (2..4096), an odd smoothing window W (1..G).
 *   A detection counts if its label is an integer in 1..K, det_match != -2 and det_ignore == 0; it is a TP
 *   if det_match >= 0, else an FP.  npos[k] = ground truths with label k+1 and true_crowd == 0.
 *   c_j = (double)j / (G-1).  tp[k,j] / fp[k,j] = counted TPs / FPs of class k+1 with (double)score >= c_j
 *   (a NaN score is counted nowhere, a score above 1 everywhere).
 *   P = tp/(tp+fp), 1.0 where tp+fp == 0; R = tp/npos; F1 = ((2.0*P)*R)/((P+R)+1e-16); with npos[k] == 0 all
 *   three are -1 and the class is left out of every mean.  mean_f1[j] = (sum of F1 over the classes with
 *   positives, ascending k, starting from 0.0) / their number, -1 without any.  smooth_f1[j] = (sum of
 *   mean_f1[clamp(i, 0, G-1)] for i = j-W/2 .. j+W/2, ascending, starting from 0.0) / W.  best = the first j
 *   that maximises smooth_f1; best_conf = c_best.  at_best[K+1,3] = (P, R, F1) of each class at best; row K =
 *   their means over the classes with positives (same order and start), -1 without any.
 *   Outputs (device): tp, fp [K,G] int64; npos[K] int64; precision, recall, f1 [K,G] fp64; mean_f1[G],
 *   smooth_f1[G] fp64; best[1] int32; best_conf[1] fp64; at_best[(K+1)*3] fp64.
 *   D == 0 and T == 0 are valid.  D, T <= 2^30; beyond the limits MNY_EINVAL with a mny_last_error text, and
 *   mny_det_curves_ws_bytes returns 0.  ws: mny_det_curves_ws_bytes(D, T, n_classes, G, W) bytes.
 *
 * mny_det_confusion.  Inputs: the packed layout of mny_coco_eval (image_sizes NULL = (1, 1)), conf and
 *   iou_thr (not NaN), accumulate (0: the matrix is zeroed first; 1: it is added to, one call per batch).
 *   Per image: the detections are those with an integer label in 1..K and (double)score > conf; the ground
 *   truths those with an integer label in 1..K, crowds included.  IoU: the geometry of mny_coco_eval with the
 *   non-crowd union for every pair.  Candidates are the pairs with iou > iou_thr (a NaN IoU is none); classes
 *   are not compared.  Repeatedly the candidate of largest IoU whose detection and ground truth are both free
 *   is taken (among equal IoUs the smaller stored detection index, then the smaller ground-truth index) and
 *   both are marked matched, until no candidate is left: at most min(detections, ground truths) rounds.
 *   matrix[(K+1),(K+1)] int64, row = predicted class, column = true class, index K = background: a matched
 *   non-crowd ground truth adds 1 at [pred-1][true-1], an unmatched non-crowd one at [K][true-1], an unmatched
 *   detection at [pred-1][K]; a crowd ground truth and the detection matched to it add nothing; [K][K] stays
 *   0.  Optional det_gt[D] (int32, stored order, NULL to skip): packed index of the matched ground truth, -1
 *   unmatched, -2 not considered.  Boxes per image have no limit (an LDS table of IoUs for small images,
 *   recomputation beyond it).  Limits: n_classes 2..255, n_images < 2^24, D, T <= 2^30; beyond them
 *   MNY_EINVAL (mny_det_confusion_ws_bytes returns 0).  ws: mny_det_confusion_ws_bytes(D, T, n_images,
 *   n_classes) bytes.
 * Both: no host sync, no floating-point atomics (integer adds only), deterministic. */
size_t mny_det_curves_ws_bytes(int64_t D, int64_t T, int n_classes, int G, int W);
int mny_det_curves(const float* det_labels, const float* det_scores, const int32_t* det_match,
                   const uint8_t* det_ignore, int64_t D, const float* true_labels, const float* true_crowd,
                   int64_t T, int n_classes, int G, int W, int64_t* tp, int64_t* fp, int64_t* npos,
                   double* precision, double* recall, double* f1, double* mean_f1, double* smooth_f1,
                   int32_t* best, double* best_conf, double* at_best, void* ws, void* stream);
size_t mny_det_confusion_ws_bytes(int64_t D, int64_t T, int n_images, int n_classes);
int mny_det_confusion(const float* det_boxes /*[D,4]*/, const float* det_labels, const float* det_scores,
                      const int32_t* det_off /*[n_images+1]*/, const float* true_boxes /*[T,4]*/,
                      const float* true_labels, const float* true_crowd, const int32_t* true_off,
                      const float* image_sizes /*[n_images,2], NULL = (1,1)*/, int n_images, int64_t D,
                      int64_t T, int n_classes, double conf, double iou_thr, int accumulate, int64_t* matrix,
                      int32_t* det_gt, void* ws, void* stream);

/* ---- segmentation head of the BDD100K config ------------------------------------------------
 * Replaces SegLoss.forward (models/seg_loss.py:51-80) and its autograd on the channels-last seg head
 * [N,h,w,C] (the reference permutes seg_maps [N,h,w,C] to NCHW instead, :54): n = N*h*w*C elements.
 * out3 = (0.05 * mean((sigmoid(x)-t)^2), mean sigmoid where t >= 0.5, mean sigmoid where t < 0.5) — an empty
 * selection gives NaN like torch.mean; dhead = 0.05*2*(sigmoid(x)-t)/n: the reference's custom sigmoid passes the
 * gradient through unchanged (:24-32).  ws: mny_seg_loss_ws_bytes(n).  Deterministic (fixed-order fp64 sums). */
size_t mny_seg_loss_ws_bytes(int64_t n);
int mny_seg_loss(const float* head, const float* seg_maps, int64_t n, float* out3, float* dhead, void* ws,
                 void* stream);
/* eval branch (:77-80): sigmoid of image 0 only, written channel-major [C,h,w] like the reference's numpy result */
int mny_seg_sigmoid(const float* head /*[N,h,w,C], image 0 is read*/, int h, int w, int C, float* out,
                    void* stream);

/* ---- segmentation evaluation on the device (csrc/segeval.hip) --------------------------------------------------
 * Scores the seg head against full-resolution ground-truth id maps: the reference has no such step (its test()
 * loader returns no seg labels, folder2lmdb.py:264-265); the prediction rule is the one of its only consumer of
 * the seg output, inference.py:64-67,100-103 (each class map resized to the image with cv2.INTER_LINEAR, then
 * > 0.5).  cv2 is restated, not linked: the arithmetic below IS the specification (tests/segeval_ref.py holds it
 * in numpy, float64); it is half-pixel bilinear resizing without antialiasing, as
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False) computes it.
 * head: DEVICE fp32 [N,h,w,C], the raw seg logits, channels last.  Image i has its own size (H_i, W_i) =
 * sizes[2i], sizes[2i+1]; sizes and the offsets are HOST arrays, read during the call (their entries travel in the
 * kernel arguments, 96 images per launch).  1 <= C <= 16; h, w, H_i, W_i in 1..16384; w * C <= 6144.
 *   p = 1 / (1 + expf(-x)) in fp32 (the sigmoid of mny_seg_sigmoid and mny_seg_loss).
 *   Output row Y reads head rows clamp(y0, 0, h-1) and clamp(y0 + 1, 0, h-1) with weight ty, where, in integers,
 *     ny = (2Y + 1) h - H_i, y0 = floor(ny / (2 H_i)), ry = ny - y0 * 2 H_i, and ty = (float)ry / (float)(2 H_i)
 *     (both exact in fp32, one rounding); columns alike with w, W_i.
 *   v = a (1 - ty) + b ty with a = p00 (1 - tx) + p01 tx, b = p10 (1 - tx) + p11 tx: every subtraction, product and
 *     sum an fp32 operation of its own (no fused multiply-add).  At H_i = h, W_i = w every weight is 0 and v = p.
 *   Predicted id: with m = max_c v_c, 0 (background) unless m > 0.5, else 1 + the lowest c with v_c == m; a NaN
 *     never wins and never passes the threshold.
 *   Ground truth: uint8 id maps, id c in 1..C = class c, 0 = background (folder2lmdb.py:140-141), an id above C
 *     (e.g. 255) = ignored.
 * mny_seg_confusion: labels / pred_out are DEVICE buffers, 16-byte aligned, image i at byte label_offsets[i] (a
 *   multiple of 16) as H_i rows of W_i bytes with NO row padding.  conf[g][pred] += 1 in the int64 [(C+1),(C+1)]
 *   DEVICE matrix and *ignored += 1 per ignored pixel: the call ADDS to what is there (integer sums: the result
 *   does not depend on launch order).  pred_out (or NULL) receives the predicted id map in the labels' layout;
 *   bytes between the images are not written.  labels may be NULL when only pred_out is wanted (conf and ignored
 *   are then not touched).  Nothing is read past an image's H_i * W_i bytes.
 * mny_seg_upsample: the interpolated probabilities v, image i as fp32 [C,H_i,W_i] at out + out_offsets[i] floats
 *   (a multiple of 4; out 16-byte aligned): a batch of what inference.py:66-67 does per class.
 * mny_seg_metrics: out (DEVICE fp64 [C+4]) = iou[0..C], miou, miou_fg, pixel_acc with
 *   iou[k] = conf[k][k] / (row_k + col_k - conf[k][k]) (NaN at a zero denominator), miou the mean of the non-NaN
 *   iou over 0..C, miou_fg over 1..C (sums in index order, NaN if there is none), pixel_acc = trace / sum.
 * No host sync, no allocation, no workspace. */
int mny_seg_confusion(const float* head /*[N,h,w,C]*/, int N, int h, int w, int C, const uint8_t* labels,
                      const int64_t* label_offsets /*HOST [N]*/, const int32_t* label_sizes /*HOST [N,2] = (H, W)*/,
                      int64_t* conf, int64_t* ignored, uint8_t* pred_out, void* stream);
int mny_seg_upsample(const float* head /*[N,h,w,C]*/, int N, int h, int w, int C,
                     const int32_t* sizes /*HOST [N,2] = (H, W)*/, const int64_t* out_offsets /*HOST [N]*/, float* out,
                     void* stream);
int mny_seg_metrics(const int64_t* conf /*[(C+1),(C+1)]*/, int C, double* out /*[C+4]*/, void* stream);

/* ---- device-side batch input preparation ------------------------------------------------------
 * Replaces the image half of collate_fn (folder2lmdb.py:223-256): per image transforms.Resize(size, BILINEAR) on
 * the decoded PIL image, ToTensor, Normalize(mean, std), torch.stack — with the batch's one
 * random.choice(train_img_size) made by the caller.  The resize is Pillow's ImagingResample (third-party, not
 * vendored): antialiased triangle filter whose support grows with the down-scale factor, 22-bit fixed-point taps,
 * horizontal pass then vertical pass, each rounded to uint8 — reproduced bit for bit; then
 * out = (u8/255 - mean)/std in fp32 (same divisions as torch).
 * src: decoded RGB uint8 images, HWC, anywhere in one device buffer; desc (DEVICE, [N]): byte offset + size of
 * each.  max_in_h/max_in_w: caller's upper bounds on the source sizes (size the workspace and the tap tables); an
 * image outside them is written as zeros and the int32 at ws+0 receives 1+its index (0 = ok).
 * mean3/std3: HOST arrays of 3 floats, read during the call.  out: [N,3,out_h,out_w] fp32 (NCHW, what
 * mny_stem_fwd reads).  ws: mny_prep_ws_bytes().  No host sync. */
typedef struct mny_image_desc {
    int64_t offset; /* bytes from src to pixel (0,0) */
    int32_t h, w;
} mny_image_desc;
size_t mny_prep_ws_bytes(int N, int max_in_h, int max_in_w, int out_h, int out_w);
int mny_prep_batch(const uint8_t* src, const mny_image_desc* desc, int N, int max_in_h, int max_in_w, int out_h,
                   int out_w, const float* mean3, const float* std3, float* out, void* ws, void* stream);

/* ---- device-side training augmentation (csrc/augment.hip) ------------------------------------------------------
 * The train-phase sample path of the reference's data pipeline, after decoding: per image transform_od
 * (image_augmentation.py:279-334: photometric_distort -> expand_od -> random_crop_od -> flip_od), for groups of
 * 2..4 images Mosaic (:216-278) on a square canvas, then collate_fn's BILINEAR resize + ToTensor + Normalize
 * (folder2lmdb.py:223-256).  Every draw is made on the host (augment.py TrainAugment.plan); the device only does
 * the pixel work, bit for bit against Pillow:
 *   photometric ops at source resolution, uint8 -> uint8 (Image.blend with a float alpha for brightness /
 *   contrast / saturation, contrast's grey = int(mean(L) + 0.5) of the image as it is at that point of the chain,
 *   Pillow RGB<->HSV for hue, a host-built 256-entry map for gamma); the geometry is read THROUGH (expand canvas
 *   with filler 127, crop window, horizontal flip) by the resample, nothing is materialised for a single image;
 *   Mosaic tiles are Pillow BICUBIC resizes (a = -0.5) pasted into a uint8 canvas whose mask rectangle is filled
 *   with trunc(sum / count) of the resized tile per channel; the final resize is Pillow BILINEAR, then
 *   out = (u8/255 - mean)/std in fp32.
 * mny_aug_item (DEVICE array, one per decoded image): src = byte offset (a multiple of 4) + size of the image in
 *   `src`; op[0..n_ops) in application order (MNY_AUG_*), factor[k] = the blend alpha of op k; hue_shift = the
 *   uint8 added to H; gamma_map = the point() table; expand: the canvas size and the image's place in it (exp_h =
 *   h, exp_w = w, exp_top = exp_left = 0 when not expanded); crop: the window inside the expanded image (all of it
 *   when not cropped); flip; sample = the output index; mosaic members also carry their tile rectangle (top-left +
 *   size of the resized image in the canvas) and mask rectangle (x0, y0, x1, y1).
 * mny_aug_sample (DEVICE array, one per output image): items [first_item, first_item + n_items); n_items 1 = a
 *   single image, 2..4 = a mosaic drawn on canvas slot `canvas_slot` (0..n_mosaic-1).
 * max_in_h/max_in_w bound every source image AND every expanded / cropped image; canvas = the mosaic side.  An
 * item outside the bounds (or a misaligned offset, an op list longer than 5, a tile outside its mask) is not read,
 * its sample is written as zeros and the int32 at ws+0 receives 1 + its index; a malformed sample record
 * receives -(1 + sample index).  mean3/std3: HOST arrays of 3 floats.  out: [n_out,3,out_h,out_w] fp32.
 * ws: mny_aug_ws_bytes() (same arguments).  No host sync, no allocation; deterministic launch to launch.
 * mny_aug_photometric: the photometric chain alone, item k writes dst + items[k].src.offset (dst laid out like
 * src); only src, the op fields and the bounds are read; ws: at least mny_aug_ws_bytes(n, 0, 0, max_in_h,
 * max_in_w, 0, 1, 1) bytes. */
#define MNY_AUG_BRIGHTNESS 0
#define MNY_AUG_CONTRAST 1
#define MNY_AUG_SATURATION 2
#define MNY_AUG_HUE 3
#define MNY_AUG_GAMMA 4
typedef struct mny_aug_item {
    mny_image_desc src;
    int32_t n_ops;
    int32_t op[5];
    float factor[5];
    int32_t hue_shift;
    uint8_t gamma_map[256];
    int32_t exp_h, exp_w, exp_top, exp_left;
    int32_t crop_top, crop_left, crop_h, crop_w;
    int32_t flip;
    int32_t sample;
    int32_t tile_x, tile_y, tile_w, tile_h;
    int32_t mask_x0, mask_y0, mask_x1, mask_y1;
} mny_aug_item; /* 392 bytes */
typedef struct mny_aug_sample {
    int32_t first_item, n_items, canvas_slot, reserved;
} mny_aug_sample;
size_t mny_aug_ws_bytes(int n_items, int n_out, int n_mosaic, int max_in_h, int max_in_w, int canvas, int out_h,
                        int out_w);
int mny_aug_photometric(const uint8_t* src, const mny_aug_item* items, int n, int max_in_h, int max_in_w,
                        uint8_t* dst, void* ws, void* stream);
int mny_aug_batch(const uint8_t* src, const mny_aug_item* items, int n_items, const mny_aug_sample* samples,
                  int n_out, int max_in_h, int max_in_w, int canvas, int n_mosaic, int out_h, int out_w,
                  const float* mean3, const float* std3, float* out, void* ws, void* stream);

/* Segmentation maps of a config with a `seg:` section (folder2lmdb.py:99-110,135-141,243-261), for the items and
 * samples of an mny_aug_batch call.  The uint8 id map of an image has the image's size and makes its geometric trip
 * (expand_od with border 0, the crop window, the flip; the photometric chain does not touch it); for c = 1..n_classes
 * the 0/255 image (id == c) is resized to [out_h,out_w] with the arithmetic of OpenCV's INTER_AREA for uchar, one
 * channel, both scales >= 1 (resize.cpp: per axis the fp64 tap table of computeResizeAreaTab with float weights,
 * horizontal fp32 sums in tap order, then sum = beta*buf / sum += beta*buf in row order, no FMA, rounded to nearest
 * even; integer scales on both axes take ResizeAreaFast's round((float)isum * (1.f/area))), and out[...,c-1] =
 * (float)u8 / 255.0f.  Id 0 and ids above n_classes land in no map.  OpenCV is restated, not linked: the resize half
 * is parity-unpinned (tests/augment_seg_ref.py holds the same definition in numpy).
 * seg_src: DEVICE uint8, 4-byte aligned; seg_offsets: DEVICE, per item the byte offset (a multiple of 4) of its
 * [h,w] id map; the bytes up to the next multiple of 4 after a map must be readable.  Of each item only src.h,
 * src.w, exp_*, crop_*, flip and sample are read.  n_classes: 1..MNY_AUG_SEG_MAX_CLASSES; out_w * n_classes <= 4096.
 * Every sample must hold exactly one item (the reference defines no Mosaic with seg maps) and its cropped geometry
 * must be at least out_h x out_w (a scale below 1 is another OpenCV path, not implemented): such a record is not
 * read, its maps are written as zeros and the int32 at ws+0 receives 1 + the item index (bad geometry, offset or
 * bounds) or -(1 + sample index) (bad record), as mny_aug_batch does.  out: [n_out,out_h,out_w,n_classes] fp32,
 * ready for mny_seg_loss.  ws: mny_aug_seg_ws_bytes() (0 = bad arguments).  No host sync, no allocation;
 * deterministic launch to launch. */
#define MNY_AUG_SEG_MAX_CLASSES 8
size_t mny_aug_seg_ws_bytes(int n_items, int n_out, int n_classes, int max_in_h, int max_in_w, int out_h, int out_w);
int mny_aug_seg_batch(const uint8_t* seg_src, const int64_t* seg_offsets, const mny_aug_item* items, int n_items,
                      const mny_aug_sample* samples, int n_out, int n_classes, int max_in_h, int max_in_w, int out_h,
                      int out_w, float* out, void* ws, void* stream);

/* ---- the loader's blur / sharpen / noise stage (csrc/augseq.hip) ----------------------------------------------
 * The reference runs imgaug's `seq` (folder2lmdb.py:28-42) on every decoded image before transform_od (:131):
 * Sometimes(0.5, SomeOf((1, 2), [OneOf([GaussianBlur(0..1), MedianBlur(3..5)]), Sharpen(alpha 0..0.1, lightness
 * 0.9..1.1), AdditiveGaussianNoise(scale 0..0.03*255, per_channel 0.3)], random_order)).  The host makes the draws
 * (augment.py SeqAugment.plan); the device applies zero, one or two ops per image, uint8 -> uint8, the second op
 * reading the first one's uint8 result.  imgaug and cv2 are restated, not linked: this stage is parity-unpinned
 * against them and the arithmetic below IS the specification (tests/seq_ref.py holds it in numpy/scipy, fp64).
 * With p the centre pixel, per channel:
 *   MNY_SEQ_GAUSS    5x5 separable (imgaug's size for sigma <= 1 is max(int(3.3 sigma), 5) = 5).  taps[d+2] =
 *                    exp(-d^2 / 2 sigma^2), d = -2..2, normalised in fp64 and cast to fp32 by the host.  Horizontal
 *                    pass sum_d taps[d] * p in fp32, in tap order, kept unrounded; vertical pass the same; rintf,
 *                    clamp to 0..255.  Border REFLECT_101 (dcb|abcd|cba), iterated, so that sides of 1 and 2 work
 *                    (a side of 1 reads index 0).  sigma < 1e-3 is the identity: the host emits no op.
 *   MNY_SEQ_MEDIAN   median_k x median_k, median_k 3 or 5, border REPLICATE, exact.
 *   MNY_SEQ_SHARPEN  rintf(sharpen_c * p + sharpen_s * S8) clamped to 0..255, S8 the integer sum of the eight
 *                    neighbours under REFLECT_101; the two products and the sum are fp32 operations of their own (no
 *                    FMA).  Host: sharpen_c = (1 - alpha) + alpha * (8 + lightness), sharpen_s = -alpha in fp64, cast
 *                    to fp32; alpha = 0 is exactly the identity.
 *   MNY_SEQ_NOISE    Philox4x32-10 as published, key = noise_key, counter = (y * w + x, 0, 0, 0); its outputs r0..r3
 *                    give u_i = ((float)(r_i >> 8) + 0.5f) * 2^-24 (in (0, 1]; exact below 2^23, else rounded to
 *                    fp32); z0 = R(u0) cos(2 pi u1), z1 = R(u0) sin(2 pi u1), z2 = R(u2) cos(2 pi u3), R(u) =
 *                    sqrtf(-2 logf(u)), accurate fp32 library functions.  noise_per_channel: the channels take z0,
 *                    z1, z2, otherwise all three take z0.  out = clamp(p + (int)rintf(noise_scale * z), 0, 255).
 * src: decoded RGB uint8 images, HWC, packed in one DEVICE buffer; desc (DEVICE, [n_items]): offset (a multiple of
 * 4) and size of each, 3 * h * w bytes; seq (DEVICE, [n_items]): one record per image.  dst is laid out like src
 * (dst != src; src, dst and ws 4-byte aligned): after the call it holds EVERY image, one with n_ops == 0 copied byte
 * for byte; bytes between and after the images are not written.  Nothing is read past an image's 3 * h * w bytes.
 * max_in_h / max_in_w: the caller's bounds on the image sizes (at most 16383); n_items at most 4096.
 * The int32 at ws+0 receives 0, or 1 + the lowest index of an item that is outside the bounds or misaligned, has
 * n_ops outside 0..2, an unknown or a repeated op, a median size other than 3 or 5, or a non-finite coefficient of
 * an op it uses.  Such an image is written as zeros (an item with a negative offset or a side outside 1..16383
 * names no bytes and is only reported); nothing outside its 3 * h * w bytes is touched.
 * ws: mny_aug_seq_ws_bytes() (0 = bad arguments; src_bytes = the size of src).  The two-op images pass through ws:
 * after the call ws + 256 + offset holds op 0's uint8 result of each of them.
 * Two launches, no host sync, no allocation, no atomics; deterministic launch to launch. */
#define MNY_SEQ_GAUSS 0
#define MNY_SEQ_MEDIAN 1
#define MNY_SEQ_SHARPEN 2
#define MNY_SEQ_NOISE 3
typedef struct mny_aug_seq_item {
    int32_t n_ops; /* 0..2 */
    int32_t op[2]; /* MNY_SEQ_*, in application order, no kind twice */
    float taps[5];
    int32_t median_k;
    float sharpen_c, sharpen_s;
    float noise_scale;
    int32_t noise_per_channel;
    uint32_t noise_key[2];
    int32_t reserved;
} mny_aug_seq_item; /* 64 bytes */
size_t mny_aug_seq_ws_bytes(int n_items, int64_t src_bytes, int max_in_h, int max_in_w);
int mny_aug_seq_batch(const uint8_t* src, const mny_image_desc* desc, const mny_aug_seq_item* seq, int n_items,
                      int max_in_h, int max_in_w, uint8_t* dst, void* ws, void* stream);

/* ---- random perspective: rotation, scale, shear, translation, perspective (csrc/augwarp.hip) -------------------
 * The geometric warp every YOLOv5-family trainer runs on every sample (random_perspective).  The reference has no
 * counterpart: its geometry is axis-aligned (expand, crop, flip, Mosaic tiles).  The host draws and inverts one 3x3
 * matrix per image (augment.py RandomPerspective.plan) and transforms the boxes; the device does the per-pixel gather,
 * uint8 -> uint8, the output the size of the input, bit for bit what Pillow's Image.transform(size, PERSPECTIVE, c,
 * BILINEAR or NEAREST, fillcolor) writes (tests/warp_ref.py restates it in numpy and is pinned to Pillow).
 * Coordinates are Pillow's continuous ones: pixel (i, j) covers [i, i+1) x [j, j+1), its centre is (i+0.5, j+0.5);
 * boxes use the same (cx * w etc.).  Everything below is fp64 without FMA contraction.
 * c[0..7]: the INVERSE map, output -> source, normalised so that the ninth coefficient is 1.  For output pixel (x, y):
 *   xi = x + 0.5, yi = y + 0.5; den = c6*xi + c7*yi + 1; xin = (c0*xi + c1*yi + c2) / den; yin = (c3*xi + c4*yi + c5) / den
 *   (sums left to right).  With c6 == c7 == 0 den is exactly 1 and the division is skipped: the same bits.  den <= 0 or a
 *   non-finite xin / yin writes the fill (Pillow defines neither case).
 * channels 3, RGB, BILINEAR (bilinear_filter32RGB): xin < 0 || xin >= w || yin < 0 || yin >= h writes the fill; otherwise
 *   xs = xin - 0.5, ys = yin - 0.5, X = floor(xs), Y = floor(ys), dx = xs - X, dy = ys - Y; x0 = clamp(X, 0, w-1), x1 =
 *   clamp(X+1, 0, w-1), row y0 = clamp(Y, 0, h-1); per channel v1 = p[y0][x0] + (p[y0][x1] - p[y0][x0]) * dx; v2 the same
 *   on row Y+1 if 0 <= Y+1 < h, else v2 = v1; v = v1 + (v2 - v1) * dy; out = (uint8)v, truncated.
 * channels 1, NEAREST (id maps; nearest_filter8): the same four comparisons in fp64, before any conversion to int, write
 *   the fill; otherwise out = p[(int)yin][(int)xin].
 * fill: (127, 127, 127) for images (expand_od's filler), fill[0] = 0 for id maps (background, as expand_od's border).
 * Host side (numpy fp64): the forward matrix is YOLOv5's composition M = T . S . R . P . C: C moves (w/2, h/2) to the
 *   origin; P[2,0] = px, P[2,1] = py; R = [[s cos a, s sin a, 0], [-s sin a, s cos a, 0], [0, 0, 1]]; S[0,1] = tan(shx),
 *   S[1,0] = tan(shy); T[0,2] = tx*w, T[1,2] = ty*h.  c = inv(M) / inv(M)[2,2], first eight entries (c6 = c7 = 0 exactly
 *   when M[2,0] = M[2,1] = 0: the inverse of an affine map is affine, whatever the solver rounds).  M == identity exactly
 *   marks the item `identity`: its image is copied byte for byte and its targets are left untouched.  Otherwise each box
 *   goes to pixel corners, the four corners go through M with the perspective divide, the new box is their min / max
 *   clipped to [0,w] x [0,h], and it is kept iff its new width > 2 px, its new height > 2 px, max(w'/h', h'/w') < 100 and
 *   area' / (area * |det M[:2,:2]| + 1e-16) > 0.1; back to (cls, cx, cy, w, h) normalised, float32.  The forward
 *   denominator M[2].(x, y, 1) must be positive at the four source corners.
 * src: the packed upload of mny_aug_seq_batch: uint8 images, HWC, in one DEVICE buffer; desc (DEVICE, [n_items]): offset
 * (a multiple of 4) and size of each, channels * h * w bytes; warp (DEVICE, [n_items]): one record per image.  dst is
 * laid out like src (dst != src; src, dst and ws 4-byte aligned): after the call it holds EVERY image, an identity item
 * copied byte for byte; bytes between and after the images are not written.  Nothing is read past an image's channels *
 * h * w bytes.  max_in_h / max_in_w: the caller's bounds on the image sizes (at most 16383); n_items at most 4096.
 * The int32 at ws+0 receives 0, or 1 + the lowest index of an item that is outside the bounds, misaligned or carries a
 * non-finite coefficient.  Such an image is written as zeros (an item with a negative offset or a side outside 1..16383
 * names no bytes and is only reported); nothing outside its bytes is touched.  That offset + channels * h * w lies inside
 * src and dst is the caller's responsibility, as for mny_aug_seq_batch.
 * ws: mny_aug_warp_ws_bytes() (0 = bad arguments).  One launch, no host sync, no allocation, no atomics; deterministic
 * launch to launch. */
typedef struct mny_aug_warp_item {
    double c[8];      /* the inverse map, output -> source */
    int32_t identity; /* non-zero: copy the image */
    uint8_t fill[3];
    uint8_t reserved;
} mny_aug_warp_item; /* 72 bytes */
size_t mny_aug_warp_ws_bytes(int n_items, int channels, int max_in_h, int max_in_w);
int mny_aug_warp_batch(const uint8_t* src, const mny_image_desc* desc, const mny_aug_warp_item* warp, int n_items,
                       int channels /* 3: RGB bilinear, 1: id map nearest */, int max_in_h, int max_in_w,
                       uint8_t* dst, void* ws, void* stream);

/* ---- baseline JPEG decode: host entropy stage, device pixel stage (csrc/jpeg_host.h, csrc/jpeg.hip) -----------
 * The reference decodes with cv2.imdecode on the loader workers (folder2lmdb.py:94) from the raw file bytes its LMDB
 * stores (:266).  Here the decode is cut where the work changes character: marker parsing and Huffman decoding stay
 * on the host (serial, branchy), everything per pixel runs on the device, and what crosses the bus is the quantised
 * coefficients as int16, 3 bytes per pixel at 4:2:0, as much as the RGB upload it replaces.  The pixel arithmetic is
 * integer work and equals libjpeg's default decode (ISLOW inverse DCT, fancy upsampling) bit for bit for streams a real
 * encoder wrote: Pillow with libjpeg-turbo is pinned by the tests; cv2.imdecode uses the same library defaults but is
 * not installed, so that one is unpinned.  For hostile coefficients the claim is memory safety and determinism only:
 * libjpeg's 64-bit intermediates and masked range table are not reproduced.
 *
 * Streams taken: SOF0, 8-bit samples, 8-bit quantisation tables; one component, or three components YCbCr (JFIF, an
 * Adobe marker with transform 1, or neither) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; one interleaved scan;
 * Huffman tables from DHT; DRI / RSTn; FF 00 stuffing and fill bytes.  Sides up to 16383.  Every other stream gets one
 * of the non-zero MNY_JPEG_* statuses below and no coefficients; a bad image never fails a call.
 *
 * mny_jpeg_probe (HOST): reads the headers up to SOS, never past data + len.  info->h, w and ncomp are filled whenever a
 *   frame header was read (also for a progressive stream); the rest only with status 0: hs, vs = the luma sampling
 *   factors (1, 1 for one component), bw[c] x bh[c] = the block grid of plane c, padded to whole MCUs, n_coef = 64 *
 *   sum bw[c] * bh[c].  Returns MNY_EINVAL for a null pointer only.
 * mny_jpeg_entropy_batch (HOST): for image i the coefficients go to coef + coef_off[i] (int16 elements; a multiple of 8
 *   so that the device loads 16 bytes), at most coef_cap[i] of them (fewer than n_coef: MNY_JPEG_ECAPACITY, nothing
 *   written).  Blocks are de-zigzagged to natural order (index 8 * row + column), the planes follow one another
 *   (plane_off), within a plane the blocks are row-major over the padded grid.  Coefficients saturate to int16.  items[i]
 *   is the record the device reads: the sizes, the planes, the three quantisation tables in natural order, the status,
 *   and coef_off[i].  n_threads is clamped to 1..16; image i is decoded by thread i mod n_threads, so the output does
 *   not depend on timing; nothing is allocated.  Nothing is read past data[i] + len[i] and nothing is written outside
 *   coef[coef_off[i] .. + coef_cap[i]); a failed image may leave part of its slice written.
 *
 * mny_jpeg_pixels_batch (DEVICE): coef and items as the host stage wrote them, copied to the device; desc (DEVICE,
 *   [n]): where each image goes in dst, offset a multiple of 16, h and w equal to the item's.  Two launches:
 *   (a) every 8x8 block of every plane: v = coef * q, then the 1-D inverse DCT below on the columns, each output
 *       (x + 1024) >> 11, then on the rows, each output (x + 131072) >> 18, sample = clamp(x + 128, 0, 255), into uint8
 *       planes in ws (ws + 256 + coef_off + plane_off, bw * 8 bytes per row).  Every shift is arithmetic, every
 *       intermediate 32-bit.  With 13-bit constants, on (v0..v7):
 *         z1 = (v2 + v6) * 4433; t2 = z1 - v6 * 15137; t3 = z1 + v2 * 6270; t0 = (v0 + v4) << 13; t1 = (v0 - v4) << 13;
 *         t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2;
 *         a0..a3 = v7, v5, v3, v1; z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3; z5 = (z3 + z4) * 9633;
 *         a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5;
 *         z4 = z4 * -3196 + z5; a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
 *         out = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
 *   (b) upsample, convert, write interleaved RGB to dst + desc[i].offset.  A chroma plane is first cropped to cw =
 *       ceil(w / 2) (2x1, 2x2) by ch = ceil(h / 2) (2x2) real samples; a neighbour beyond an edge is the edge sample.
 *         2x1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2
 *         2x2: output row 2j takes s[i] = 3 p[j][i] + p[j-1][i], row 2j+1 takes s[i] = 3 p[j][i] + p[j+1][i]; then
 *              out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4
 *         cw <= 2: libjpeg does not filter such a plane, out[y][x] = p[y >> 1][x >> 1] (2x2) or p[y][x >> 1] (2x1)
 *       and the result is cropped to h x w.  With cb -= 128, cr -= 128: r = y + ((91881 cr + 32768) >> 16), g = y +
 *       ((-22554 cb - 46802 cr + 32768) >> 16), b = y + ((116130 cb + 32768) >> 16), each clamped to 0..255.  One
 *       component writes y three times.
 *   The int32 at ws+0 receives 0, or 1 + the lowest index of an item that is not sound: a non-zero status; sizes,
 *   sampling, block grids, plane offsets or n_coef that do not agree with each other; coef_off negative or not a multiple
 *   of 8; desc offset negative or not a multiple of 16; desc h, w different from the item's or above max_h, max_w.  Such
 *   an image is neither read nor written: its bytes in dst are left for the caller's fallback decoder to fill.  Nothing
 *   outside an image's 3 * h * w bytes is touched.  n at most 4096.  coef and ws 16-byte aligned.
 *   What the kernels canNOT check is an upper bound: the call carries neither the size of coef nor that of dst, so that
 *   coef_off + n_coef <= coef_elems for every item (the same range, in bytes, is the item's planes in ws) and that
 *   desc offset + 3 * h * w lies inside dst are the caller's responsibility, as the size of dst is for mny_aug_seq_batch.
 *   Records that mny_jpeg_entropy_batch wrote satisfy the first whenever its coef_off / coef_cap slices lie inside coef.
 *   ws: mny_jpeg_ws_bytes(n, coef_elems), coef_elems = the int16 count of the coef buffer (0 = bad arguments).
 *   No host sync, no allocation, no atomics; deterministic launch to launch. */
#define MNY_JPEG_OK 0
#define MNY_JPEG_ETRUNCATED 1   /* the data ends inside the headers or before the last MCU */
#define MNY_JPEG_ENOTJPEG 2     /* no SOI */
#define MNY_JPEG_EPROGRESSIVE 3 /* SOF2 */
#define MNY_JPEG_EEXTENDED 4    /* SOF1 */
#define MNY_JPEG_EARITHMETIC 5  /* arithmetic, lossless or differential frames */
#define MNY_JPEG_EPRECISION 6   /* 12-bit samples or 16-bit quantisation tables */
#define MNY_JPEG_ECOLORSPACE 7  /* CMYK / YCCK, RGB by Adobe transform or component ids, 2 components */
#define MNY_JPEG_ESAMPLING 8    /* 4:4:0 and every other sampling outside 1x1, 2x1, 2x2 */
#define MNY_JPEG_EMULTISCAN 9   /* the first scan does not hold every component */
#define MNY_JPEG_EHUFFMAN 10    /* a code that is not in the table, a run past coefficient 63, an overfull table */
#define MNY_JPEG_EMARKER 11     /* an unexpected marker, or one that is missing (RSTn, a table, SOF before SOS) */
#define MNY_JPEG_EHEADER 12     /* a segment that contradicts itself */
#define MNY_JPEG_ETOOLARGE 13   /* a side above 16383 */
#define MNY_JPEG_ECAPACITY 14   /* the caller's coefficient slice is too small, or a null / negative argument */
typedef struct mny_jpeg_info {
    int32_t status; /* MNY_JPEG_* */
    int32_t h, w, ncomp;
    int32_t hs, vs; /* luma sampling factors */
    int32_t bw[3], bh[3];
    int64_t n_coef;
} mny_jpeg_info; /* 56 bytes */
typedef struct mny_jpeg_item {
    int32_t status;
    int32_t h, w, ncomp;
    int32_t hs, vs;
    int32_t bw[3], bh[3];
    int64_t coef_off;     /* int16 elements from coef to plane 0 */
    int64_t n_coef;
    int64_t plane_off[3]; /* int16 elements from plane 0 */
    int32_t reserved0[2];
    uint16_t q[3][64];    /* per component, natural order; byte 96 of the record, so a row of 8 is one 16-byte load */
    int32_t reserved[8];
} mny_jpeg_item; /* 512 bytes */
int mny_jpeg_probe(const uint8_t* data, int64_t len, mny_jpeg_info* info);
int mny_jpeg_entropy_batch(const uint8_t* const* data, const int64_t* len, int n, int16_t* coef,
                           const int64_t* coef_off, const int64_t* coef_cap, mny_jpeg_item* items, int n_threads);
size_t mny_jpeg_ws_bytes(int n, int64_t coef_elems);
int mny_jpeg_pixels_batch(const int16_t* coef, const mny_jpeg_item* items, int n, uint8_t* dst,
                          const mny_image_desc* desc, int max_h, int max_w, void* ws, void* stream);

/* ---- baseline JPEG encode: device coefficient stage, host entropy stage (csrc/jpegenc.hip, csrc/jpegenc_host.h) -----------
 * The way out of the device pipeline (the reference's inference.py:104 writes its result with cv2.imwrite): the decoder's
 * mirror image, cut at the same place.  Everything per pixel runs on the device and leaves quantised coefficients as int16 in
 * the layout mny_jpeg_pixels_batch reads (natural order, planes one after another, blocks row-major over the padded grid);
 * one copy takes them to the host, where Huffman coding, serial and branchy, runs threaded over the images.  All arithmetic
 * is integer work with arithmetic shifts, and the stream is byte for byte the file libjpeg-turbo writes with its defaults
 * (Pillow's Image.save(f, "JPEG", quality=Q, subsampling=S), pinned by the tests; tests/jpegenc_ref.py restates both stages
 * in numpy).  Baseline, 8-bit, three components YCbCr; luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), chroma 1x1; the
 * typical Huffman tables of Annex K.3, not optimised; quality 1..100; sides up to 16383.
 *
 * mny_jpeg_enc_layout (HOST): desc (HOST, [n]) gives h and w of each image (its offset is not read).  items[i] becomes the
 *   record of image i as the decoder defines it: ncomp 3, hs, vs, the padded block grids bw x bh (whole MCUs), plane_off,
 *   n_coef, and coef_off = the sum of the n_coef in front of it (multiples of 64), *coef_elems = their total.  q[0] is the
 *   luminance table, q[1] = q[2] the chrominance table: the tables of Annex K.1 scaled by s = 5000 / Q for Q < 50, else
 *   200 - 2 Q, each entry clamp((base * s + 50) / 100, 1, 255), integer division.  An image with a side below 1 gets status
 *   MNY_JPEG_EHEADER, one above 16383 MNY_JPEG_ETOOLARGE, and no coefficients.  MNY_EINVAL: null pointer, n outside 1..4096,
 *   quality outside 1..100, sampling other than the three above.
 *
 * mny_jpeg_coef_batch (DEVICE): src / desc (DEVICE, [n]) = packed uint8 RGB, HWC, offsets multiples of 16; items as
 *   mny_jpeg_enc_layout wrote them, copied to the device.  One launch.  For component c of size wc x hc (luma: w x h; chroma:
 *   ceil(w / hs) x ceil(h / vs)) only the blocks of its OWN grid, ceil(wc / 8) x ceil(hc / 8), are computed and written; the
 *   other blocks of the padded grid are not touched (the host stage codes them without reading them).  Per sample:
 *     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *     Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *     Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
 *   A full-resolution plane repeats its last column and its last row over its own block grid.  Chroma 2x1, output column x:
 *   (a + b + (x & 1)) >> 1 over input columns 2x, 2x + 1, a column beyond the image being the last one; rows as for a full
 *   plane.  Chroma 2x2: (a + b + c + d + 1 + (x & 1)) >> 2 over input columns 2x, 2x + 1 and rows 2y, 2y + 1, a column or row
 *   beyond the image being the last one, for y < ceil(h / 2); below that the last DOWN-SAMPLED row is repeated (for an even h
 *   that is not what repeated input rows would give).  Then per 8x8 block: sample - 128, libjpeg's accurate integer forward
 *   DCT on the rows, then on the columns, with the 13-bit constants of mny_jpeg_pixels_batch.  On (d0..d7):
 *     t0 = d0 + d7; t7 = d0 - d7; t1 = d1 + d6; t6 = d1 - d6; t2 = d2 + d5; t5 = d2 - d5; t3 = d3 + d4; t4 = d3 - d4;
 *     t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2;
 *     out0 = t10 + t11; out4 = t10 - t11: `<< 2` in the row pass, rounded `>> 2` in the column pass;
 *     z1 = (t12 + t13) * 4433; out2 = z1 + t13 * 6270; out6 = z1 - t12 * 15137;
 *     z1 = t4 + t7; z2 = t5 + t6; z3 = t4 + t6; z4 = t5 + t7; z5 = (z3 + z4) * 9633;
 *     t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5;
 *     z4 = z4 * -3196 + z5; out7 = t4 + z1 + z3; out5 = t5 + z2 + z4; out3 = t6 + z2 + z3; out1 = t7 + z1 + z4;
 *     out1, 2, 3, 5, 6, 7 rounded `>> 11` in the row pass and `>> 15` in the column pass; rounding is (x + (1 << (n-1))) >> n.
 *   Quantise: d = 8 q; c = sign(v) * ((|v| + (d >> 1)) / d).  Every intermediate fits 32 bits.
 *   The int32 at ws+0 receives 0, or 1 + the lowest index of an item that is not sound: a non-zero status; ncomp other than
 *   3; sizes, sampling, block grids, plane offsets or n_coef that do not agree with each other; a table entry outside
 *   1..255; coef_off negative or not a multiple of 8; desc offset negative or not a multiple of 16; desc h, w different
 *   from the item's or above max_h, max_w.  Such an image is neither read nor written.  As for mny_jpeg_pixels_batch the
 *   upper bounds (desc offset + 3 h w inside src, coef_off + n_coef inside coef) are the caller's responsibility; the records
 *   of mny_jpeg_enc_layout satisfy the second for a coef of *coef_elems elements.  n at most 4096; src, items, coef and ws
 *   16-byte aligned; ws: mny_jpeg_enc_ws_bytes(n) (0 = bad n).  No host sync, no allocation, no atomics; deterministic.
 *
 * mny_jpeg_huffman_batch (HOST): coef (coef_elems int16, on the host) and items as above; the stream of image i goes to
 *   out + out_off[i], at most out_cap[i] bytes, out_len[i] = its length, status[i] = MNY_JPEG_OK; every other status leaves
 *   out_len[i] = 0.  A slice that is too small gives MNY_JPEG_ECAPACITY (part of the slice may be written, nothing past it),
 *   as does a negative out_off / out_cap or a coefficient slice outside coef.  A record that is not sound (the rules above)
 *   gives its own status, MNY_JPEG_ECOLORSPACE, _ESAMPLING, _ETOOLARGE, _EPRECISION (a table entry outside 1..255) or
 *   _EHEADER.  The stream: SOI; APP0 JFIF 1.01, no density (units 0, 1 x 1), no thumbnail; DQT table 0; DQT table 1; SOF0
 *   with component ids 1, 2, 3 and tables 0, 1, 1; DHT DC 0, AC 0, DC 1, AC 1; SOS; one interleaved scan; EOI.  A block of an
 *   MCU outside its component's own grid is coded as all-zero AC with the DC of the block coded just before it in that MCU
 *   (libjpeg's rule; the transform of padded samples would give other bytes).  DC differences per component; ZRL for runs
 *   above 15, EOB unless coefficient 63 is non-zero; FF is followed by 00; the last byte is filled with ones.  A DC
 *   difference beyond 11 bits or an AC coefficient beyond 10 has no baseline code: MNY_JPEG_EHUFFMAN (libjpeg raises an
 *   error there); pixels never produce one.  n_threads is clamped to 1..16, image i is coded by thread i mod n_threads, so
 *   the output does not depend on timing; nothing is allocated.  A worst case of 420 bytes per block of the padded grids
 *   plus 700 for the headers always fits. */
int mny_jpeg_enc_layout(const mny_image_desc* desc, int n, int quality, int hs, int vs, mny_jpeg_item* items,
                        int64_t* coef_elems);
size_t mny_jpeg_enc_ws_bytes(int n);
int mny_jpeg_coef_batch(const uint8_t* src, const mny_image_desc* desc, const mny_jpeg_item* items, int n, int max_h,
                        int max_w, int16_t* coef, void* ws, void* stream);
int mny_jpeg_huffman_batch(const int16_t* coef, int64_t coef_elems, const mny_jpeg_item* items, int n, uint8_t* out,
                           const int64_t* out_off, const int64_t* out_cap, int64_t* out_len, int32_t* status,
                           int n_threads);

/* ---- annotation: draw records, then source + box outlines and labels + seg overlay into uint8 images (csrc/viz.hip) -----
 * The reference's inference product (inference.py:58-104) draws the kept boxes on the decoded image and dims the
 * drivable-area pixels; YOLO trainers write train_batch*.jpg / val_batch*_pred.jpg the same way.  Here both run on the
 * device, on what the other stages left there, and the result feeds mny_jpeg_coef_batch.  Class names and scores
 * (inference.py:90-95) are drawn from coverage strips the caller renders once with its font (mny_viz_labels,
 * mny_viz_compose_labels); the library holds no font.  No host sync, no allocation, no atomics; deterministic;
 * tests/viz_ref.py and tests/vizlabel_ref.py restate the entry points in numpy.
 *
 * mny_viz_boxes: rows / seg_begin / seg_count / S / capacity as mny_nms_per_class takes them; dims (DEVICE, [S]): h and w of
 *   the image of segment s (offset is not read).  Record i belongs to row i: nothing is compacted, no count comes back; rows
 *   outside every segment keep what `out` held.  A segment is clipped to 0 .. capacity.
 *   mode 0: rows [.,7] = (x1, y1, x2, y2, conf, cls_score, cls), normalised (mny_yolo_decode); drawn iff conf * cls_score >
 *           thr, one fp32 product, strict (inference.py:83); a NaN fails.
 *   mode 1: rows [.,5] = (cls, cx, cy, w, h), normalised (mny_yolo_loss's targets); always drawn; x1 = cx - 0.5f * w,
 *           x2 = cx + 0.5f * w, y1 = cy - 0.5f * h, y2 = cy + 0.5f * h, one fp32 operation each.
 *   Corners: floor(v * W + 0.5f) for x, floor(v * H + 0.5f) for y, in fp32 without contraction, clamped to +-2^30, then
 *   ordered: x0 = min, x1 = max, likewise y.  Colour = palette[(int)cls mod P] (DEVICE, P x 3 RGB bytes); t = thickness, 1..8.
 *   A row that fails the gate, has a NaN corner, or a class that is NaN, negative or >= 2^24 leaves the EMPTY record (t = 0).
 *
 * mny_viz_compose: item n -> h x w pixels of 3 bytes (RGB) at dst + dst_offset + y * dst_stride + 3 * x: tiles of one contact
 *   sheet or separate images; bytes between the rows of an item are not touched.  Three steps, the reference's order:
 *   1. source.  batch != NULL: fp32 [N,3,H,W], normalised as mny_prep_batch leaves it; channel c of a pixel is
 *        clamp(floor((x * std3[c] + mean3[c]) * 255 + 0.5), 0, 255): multiply, add, multiply, add in fp32, no contraction; NaN
 *        gives 0.  mean3 / std3: HOST arrays, read during the call.  Else src + desc (DEVICE, [N]): packed uint8 HWC, copied.
 *   2. boxes != NULL: the records boxes[seg_begin[n] .. + seg_count[n]) (clipped to 0 .. capacity), in order, later over
 *        earlier.  Pixel (x, y) takes a record's colour iff t > 0 and
 *          x0 <= x <= x1 and y0 <= y <= y1 and (x < x0 + t or x > x1 - t or y < y0 + t or y > y1 - t).
 *        For a box whose two sides are both at least 2 t pixels this is Pillow's ImageDraw.rectangle(outline=, width=t), parts
 *        outside the image included.  A thinner box is filled by this rule, where Pillow's result differs: for those the
 *        rule IS the specification.
 *   3. C > 0: seg + seg_offset = fp32 planes [C,h,w] of the item (mny_seg_upsample).  For class c in order, a pixel with
 *        p > 0.5f gets v = trunc((float)v * (1.0f - p)) in channel seg_channel[c] (HOST, [C], values 0..2; inference.py:100-
 *        103 in RGB terms is (1, 0)), a negative product giving 0.  C at most 8.
 *   The int32 at ws+0 receives 0, or 1 + the lowest index of an item that is not sound: a side outside 1..16383, a negative
 *   dst_offset (or seg_offset with C > 0), dst_stride below 3 w, sizes that differ from H, W or from desc[n], a negative desc
 *   offset.  Such an item is neither read nor written.  Upper bounds are the caller's.  ws: mny_viz_ws_bytes(N) (0 = N
 *   outside 1..4096).  A workgroup owns a 64 x 16 pixel tile; it filters the item's records whose outline meets the tile
 *   into a list in LDS, 256 records per pass, and its pixels walk only that list. */
typedef struct mny_viz_box {
    int32_t x0, y0, x1, y1; /* inclusive pixel corners, ordered */
    uint8_t rgb[3];
    uint8_t t;              /* thickness; 0 = empty record */
} mny_viz_box; /* 20 bytes */
typedef struct mny_viz_item {
    int64_t dst_offset; /* bytes from dst to pixel (0,0) */
    int64_t dst_stride; /* bytes from one row to the next */
    int64_t seg_offset; /* floats from seg to the item's [C,h,w] planes */
    int32_t h, w;
} mny_viz_item; /* 32 bytes */
int mny_viz_boxes(const float* rows, int mode, const int32_t* seg_begin, const int32_t* seg_count, int S, int capacity,
                  const mny_image_desc* dims, float thr, const uint8_t* palette, int P, int thickness, mny_viz_box* out,
                  void* stream);
size_t mny_viz_ws_bytes(int N);
int mny_viz_compose(const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                    const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes,
                    const int32_t* seg_begin, const int32_t* seg_count, int capacity, const float* seg, int C,
                    const int32_t* seg_channel, uint8_t* dst, void* ws, void* stream);

/* ---- annotation, text: "name score" on every drawn box (csrc/viz.hip) ----------------------------------------------------
 * The strip atlas (DEVICE, the caller's, rendered once with any font): n_names + 12 coverage strips of one line height h,
 * strip k a uint8 [h, w_k] image, row-major, at atlas + strips[2 k], with w_k = strips[2 k + 1] (strips: DEVICE, int32
 * [n_names + 12, 2]).  Strips 0 .. n_names - 1 are the class names rendered whole (a font may kern, or reach outside a
 * character's cell); strips n_names + 0 .. + 11 are the single characters "0123456789. " in that order.  Coverage 0 is
 * background, 255 is ink.  Limits: h in 1..MNY_VIZ_MAX_TEXT_H, n_names in 0..MNY_VIZ_MAX_NAMES (checked); every w_k in
 * 0..MNY_VIZ_MAX_STRIP_W and every strip inside the atlas (the caller's: the table is on the device).
 *
 * mny_viz_labels: rows / mode / seg_begin / seg_count / S / capacity / dims as mny_viz_boxes took them, and boxes = the
 *   records it wrote.  Label record i sits beside box record i: nothing is compacted, no count comes back, rows outside
 *   every segment keep what `out` held.  The label is EMPTY (48 zero bytes; n = 0) where boxes[i] is empty (t = 0: the
 *   gate is decided once, by mny_viz_boxes), in mode 1 when label_targets is 0, and where the row's class is NaN,
 *   negative or >= 2^24 (which no row of a drawn record is).  Otherwise:
 *   strips: seq[0 .. n).  c = (int)cls.  c < n_names: the one strip c.  Else the decimal digits of c, most significant first,
 *     no leading zeros (strips n_names + digit): at most 8, as c < 2^24.  In mode 0 with with_score != 0 five more follow:
 *     with k = rint((double)(conf * cls_score) * 100.0) clamped to 0..999, where conf * cls_score is the one fp32 product of
 *     the gate, the product by 100 is exact in fp64 and rint rounds ties to even, the strips of ' ', k / 100, '.',
 *     k / 10 % 10, k % 10.  For a product below 9.995 these are the characters of printf("%.2f").  n is at most
 *     MNY_VIZ_LABEL_STRIPS = 8 + 5.
 *   size: tw = the sum of the n strip widths; lw = tw + 2 * pad with pad = 2; lh = h.
 *   place (int32, from the box record's x0, y0 and the segment's dims.w = W): ly = y0 - lh if that is >= 0, else y0 (the
 *     label hangs inside the box); lx = max(min(x0, W - lw), 0).
 *   colours: bg = the box record's rgb; fg = text_rgb (HOST, 3 bytes, read during the call); filled = (filled != 0).
 *
 * mny_viz_compose_labels: mny_viz_compose with labels (DEVICE, beside boxes: labels[seg_begin[n] + r] belongs to
 *   boxes[seg_begin[n] + r]), the atlas and its table.  labels == NULL: mny_viz_compose, byte for byte (atlas and strips are
 *   not read).  labels != NULL needs boxes, atlas and strips.  Step 2 becomes, per record in order:
 *   a. the record's outline, by the rule of mny_viz_compose;
 *   b. its label, if n > 0: for a pixel (x, y) of the item with lx <= x < lx + lw and ly <= y < ly + lh,
 *        under = bg[ch] if filled, else the pixel's channel as step 1, the earlier records and (a) left it;
 *        m = coverage at text column c = x - lx - pad, row y - ly: 0 for c < 0 or c >= tw, else the byte of the strip of seq
 *            that holds column c when the n strips are laid side by side;
 *        tmp = m * fg[ch] + (255 - m) * under + 128;  channel = ((tmp >> 8) + tmp) >> 8
 *      (Pillow's ImageDraw.text through an 8-bit mask: m = 0 leaves `under`, m = 255 gives fg).  For a filled label this is
 *      ImageDraw.rectangle([lx, ly, lx + lw - 1, ly + lh - 1], fill=bg) then ImageDraw.text((lx + pad, ly), s, fill=fg),
 *      byte for byte, when the strips compose to Pillow's rendering of s (they do for ImageFont.load_default_imagefont()).
 *   Later records draw over earlier ones, labels included; step 3 (the seg overlay) follows all of them and dims label
 *   pixels too.  Pixels outside the item are never written: a label clips to its image or sheet tile.  A workgroup lists a
 *   record when its outline or its label rectangle meets the tile, and walks its list forwards. */
#define MNY_VIZ_LABEL_STRIPS 13
#define MNY_VIZ_MAX_TEXT_H 64
#define MNY_VIZ_MAX_STRIP_W 1024
#define MNY_VIZ_MAX_NAMES 4096
typedef struct mny_viz_label {
    int32_t lx, ly;                     /* top-left pixel of the label rectangle */
    int32_t lw;                         /* tw + 2 * pad */
    uint16_t seq[MNY_VIZ_LABEL_STRIPS]; /* strip indices, left to right */
    uint8_t n;                          /* strips used; 0 = empty record */
    uint8_t lh;
    uint8_t filled;                     /* 1: the rectangle is filled with bg first */
    uint8_t bg[3], fg[3];
    uint8_t reserved;                   /* 0 */
} mny_viz_label; /* 48 bytes */
int mny_viz_labels(const float* rows, int mode, const int32_t* seg_begin, const int32_t* seg_count, int S, int capacity,
                   const mny_image_desc* dims, const mny_viz_box* boxes, const int32_t* strips, int n_names, int h,
                   int with_score, int filled, int label_targets, const uint8_t* text_rgb, mny_viz_label* out,
                   void* stream);
int mny_viz_compose_labels(const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                           const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes,
                           const int32_t* seg_begin, const int32_t* seg_count, int capacity, const float* seg, int C,
                           const int32_t* seg_channel, uint8_t* dst, void* ws, const mny_viz_label* labels,
                           const uint8_t* atlas, const int32_t* strips, void* stream);

/* ---- bf16 STORAGE twins (BASELINE config 4: MobileNetV3-YOLO 512x512 bf16) -----------------
 * Every `mny_X_bf16` has the contract of `mny_X` above with ONE difference: the activation-sized tensors (the
 * `void*` parameters: raw conv outputs, materialised sums, gradients wrt activations) are bf16 in HBM.  Kernels
 * widen on load, compute and accumulate in fp32 and round once (RNE) on store; BN statistics are taken over the
 * ROUNDED outputs (what the consumer will read).  Weights, biases, view coefficients, statistics, workspaces and
 * parameter gradients stay fp32, so optimizers/checkpoints are unchanged.  The detection heads are converted to
 * fp32 (mny_cvt_bf16_f32) before mny_yolo_loss / mny_yolo_decode, whose gradient re-enters through
 * mny_cvt_f32_bf16.  Channel counts need the same alignment as the fp32 entry points (C % 4 == 0 for the
 * stencil / elementwise kernels; any K, N for the pointwise GEMMs).                                          */
int mny_stem_fwd_bf16(const float* x_nchw, const float* w, void* y, float* stats, int N, int H, int W, int Cout, void* stream);
int mny_stem_wgrad_bf16(const float* x_nchw, const void* dy, float* dw, float* ws, int N, int H, int W, int Cout, void* stream);
int mny_dw_fwd_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const float* w, void* y,
                    float* stats, int N, int H, int W, int C, int K, int stride, void* stream);
int mny_dw_bwd_data_bf16(const void* dy, const float* w, const void* addend, void* dx, int N, int H, int W, int C, int K,
                         int stride, void* stream);
int mny_dw_bwd_weight_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* dy,
                           float* dw, float* ws, int N, int H, int W, int C, int K, int stride, void* stream);
/* the pointwise GEMM also takes its WEIGHTS in bf16 ([Nc][K], e.g. mny_cvt_f32_bf16 of the fp32 master copy, or
 * mny_transpose_bf16 for the data-gradient): K % 8 == 0 runs LDS-DMA + v_mfma_f32_32x32x16_bf16, other K the
 * register-staged fp32-MFMA kernel */
int mny_pw_fwd_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* w_bf16,
                    const float* bias, const void* addend, void* y, float* stats, int64_t M, int K, int Nc, void* stream);
int mny_transpose_bf16(const float* src /*[R][Cc] fp32*/, void* dst /*[Cc][R] bf16*/, int R, int Cc, void* stream);
int mny_pw_stat_parts_bf16(int64_t M, int K, int Nc);
int mny_pw_wgrad_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* dy, float* dw,
                      float* dbias, float* ws, int64_t M, int K, int Nc, void* stream);
int mny_bn_bwd_reduce_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* mean,
                           const float* invstd, float* red, int64_t M, int C, void* stream);
int mny_bn_bwd_apply_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* coef,
                          void* dy, int64_t M, int C, void* stream);
int mny_add_views_bf16(const void* a, const float* a_scale, const float* a_shift, int a_act, const void* b,
                       const float* b_scale, const float* b_shift, int b_act, const void* up, void* out, int N, int H, int W,
                       int C, void* stream);
int mny_mul_views_bf16(const void* a, const float* a_scale, const float* a_shift, int a_act, const void* b,
                       const float* b_scale, const float* b_shift, int b_act, void* out, int64_t M, int C, void* stream);
int mny_mul_views_bwd_bf16(const void* g, const void* o, const float* o_scale, const float* o_shift, int o_act,
                           const void* addend, void* dst, int64_t M, int C, void* stream);
int mny_partadd_up_bf16(const void* a, const float* a_scale, const float* a_shift, int a_act, const void* up, void* out,
                        int N, int H, int W, int Ca, int Cb, void* stream);
int mny_slice_channels_bf16(const void* src, void* dst, int accumulate, int64_t M, int Ca, int Cb, void* stream);
int mny_upsample_bwd_bf16(const void* src, void* dst, int accumulate, int N, int H, int W, int C, void* stream);
int mny_dw_bnbwd_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* coef,
                      const void* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                      const void* addend, void* dx, float* dw, float* ws, int N, int H, int W, int C, int K, int stride,
                      void* stream);
int mny_dw_bnbwd_s2_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* coef,
                         const void* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                         const void* addend, void* dx, float* dw, float* ws, int N, int H, int W, int C, void* stream);
int mny_dw_bnbwd_red_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* coef,
                          const void* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean,
                          const float* in_invstd, const float* w, const void* addend, void* dx, float* dw, float* ws, float* in_red,
                          int N, int H, int W, int C, int K, int stride, void* stream);
int mny_pad_rows_bf16(const float* src, const float* alpha, void* dst, int64_t M, int C, int Cp, void* stream);
int mny_transpose_pad_bf16(const float* src, void* dst, int R, int Cc, int Rp, void* stream);
int mny_stem_bnwgrad_bf16(const float* x_nchw, const void* g, const void* y, const float* scale, const float* shift, int act,
                          const float* coef, float* dw, float* ws, int N, int H, int W, int Cout, void* stream);
/* fused BN-backward + weight gradient + data gradient of a thin expand unit (mny_pw_bnbwd) under bf16 storage: g, y, x, addend, dx are
 * bf16; w, statistics, dw / dgamma / dbeta and the workspace (mny_pw_bnbwd_ws_floats) fp32.  K in {8,16,24,32}, N in {64,72,96,144,192}:
 * the ReLU expand units of models/mobilenetv3.py:44-74 (16->64, 24->72) and the ReLU6 ones of models/mobilenetv2.py:75-77. */
int mny_pw_bnbwd_supported_bf16(int64_t M, int K, int Nc);
int mny_pw_bnbwd_bf16(const void* g, const void* y, const float* scale, const float* shift, int act, const float* mean, const float* invstd,
                      const float* gamma, const void* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                      const void* addend, void* dx, float* dw, float* dgamma, float* dbeta, float* ws, int64_t M, int K, int Nc, void* stream);
int mny_pw_dgrad_bnred_supported_bf16(int64_t M, int K, int Nc, int act);
int mny_pw_dgrad_bnred_parts_bf16(int64_t M, int K, int Nc);
int mny_pw_dgrad_bnred_bf16(const void* dy, const void* wT, void* dx, const void* y, const float* scale, const float* shift, int act,
                            const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream);
int mny_pw_dgrad_bnred_add_supported_bf16(int64_t M, int K, int Nc, int act);
int mny_pw_dgrad_bnred_add_bf16(const void* dy, const void* wT, const void* addend, void* dx, const void* y, const float* scale,
                                const float* shift, int act, const float* mean, const float* invstd, float* red, int64_t M, int K,
                                int Nc, void* stream);
int mny_transpose_batch_bf16(const mny_transpose_job* jobs, const int32_t* block_job, int nblocks, void* stream);
int mny_pw_wgrad_splits_bf16(int64_t M, int K, int Nc);
int mny_axpy_bf16(const void* src, const float* alpha, void* dst, int accumulate, int64_t n, void* stream);
/* all bf16 weight shadows of a forward pass in one launch: block_job maps a workgroup (4096 elements) to its job */
typedef struct mny_cvt_job {
    const float* src;
    void* dst; /* bf16 */
    int64_t n;
    int32_t block0, pad_;
} mny_cvt_job;
int mny_cvt_batch_f32_bf16(const mny_cvt_job* jobs, const int32_t* block_job, int nblocks, void* stream);
/* element-wise storage conversion, n elements (RNE to bf16, exact widening back) */
int mny_cvt_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int mny_cvt_bf16_f32(const void* src, float* dst, int64_t n, void* stream);

/* ---- frozen BatchNorm: a module in eval() whose losses are differentiated (models/mbv2_yolo.py:157 returns losses with a graph under
 * model.eval(); nn.BatchNorm2d then normalises with the running statistics, which are constants of the step).  mny_bn_eval_stats fills
 * the mean / invstd the backward kernels read (mean = running_mean, invstd = 1 / sqrt(running_var + eps)); mny_bn_bwd_finalize_frozen
 * has mny_bn_bwd_finalize's argument list and yields dgamma = sum dz * yhat, dbeta = sum dz, coef = (gamma * invstd, 0, 0). */
int mny_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean_out, float* invstd_out, int C,
                      void* stream);
int mny_bn_bwd_finalize_frozen(const float* red, int parts, int64_t count, const float* gamma, const float* mean, const float* invstd,
                               float* dgamma, float* dbeta, float* coef, int C, void* stream);
/* ---- expand + depthwise as one unit (csrc/exdw.hip): the front half of an inverted-residual block whose depthwise conv has
 * stride 2 — 1x1 conv K -> C = 6K (K in {16, 24, 32}) + BN + ReLU6 + depthwise 3x3 stride 2 (models/mobilenetv2.py:73-85) — with the
 * 6x-wide expand output and its gradient NEVER materialised: every pass recomputes it from the thin input x[N,H,W,K] (a view:
 * in_scale / in_shift / in_act as everywhere), bit-identical to what mny_pw_fwd would have stored.  fp32 storage, even H and W.
 *   mny_exdw_stats : BN batch statistics of the expand output -> partial rows [mny_exdw_stat_parts()][2][C] for mny_bn_finalize;
 *                    derived from the K x K second-moment matrix and the column sums of the viewed input (sum y^2 = w^T (x^T x) w, fp64
 *                    per workgroup): one read of x, no recomputation of y.  MNY_EXDW_STATS=direct sums the recomputed y instead.
 *   mny_exdw_fwd   : z[N,H/2,W/2,C] = dw3x3_s2(relu6(e_scale * (x w_exp^T) + e_shift)), z statistics -> [mny_exdw_fwd_parts()][2][C]
 *   mny_exdw_bwd   : given gz = dL/d act(z_scale z + z_shift) and the depthwise unit's BN-backward coefficients z_coef[3][C]
 *                    (mny_bn_bwd_finalize): dw_dw[C,3,3] (or, dw_dw == NULL, partial rows [mny_exdw_bwd_parts()][C*9] left in dw_ws),
 *                    the expand unit's dw_exp[C,K], dgamma_e, dbeta_e, and dx[N,H,W,K] = data gradient wrt the viewed input (+ addend).
 *                    ws: mny_exdw_bwd_ws_floats() floats; dw_ws: mny_exdw_bwd_parts() * C * 9 floats.  addend must NOT alias dx
 *                    (two passes: dx is overwritten before the addend is read) — MNY_EINVAL. */
int mny_exdw_supported(int N, int H, int W, int K, int C, int stride);
int mny_exdw_stat_parts(int64_t M, int K, int C);
int mny_exdw_stats(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w_exp, float* stats,
                   int64_t M, int K, int C, void* stream);
int mny_exdw_fwd_parts(int N, int H, int W, int K, int C, int stride);
int mny_exdw_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w_exp,
                 const float* e_scale, const float* e_shift, const float* w_dw, float* z, float* z_stats,
                 int N, int H, int W, int K, int C, int stride, void* stream);
int mny_exdw_bwd_parts(int N, int H, int W, int K, int C, int stride);
size_t mny_exdw_bwd_ws_floats(int N, int H, int W, int K, int C, int stride);
int mny_exdw_bwd(const float* gz, const float* z, const float* z_scale, const float* z_shift, int z_act, const float* z_coef,
                 const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w_exp,
                 const float* e_scale, const float* e_shift, const float* e_mean, const float* e_invstd, const float* e_gamma,
                 const float* w_dw, const float* addend, float* dx, float* dw_exp, float* dgamma_e, float* dbeta_e,
                 float* dw_dw, float* dw_ws, float* ws, int N, int H, int W, int K, int C, int stride, void* stream);
/* the same where x is the RAW output of a conv+BN(+act) unit consumed only by this one (view in_scale / in_shift / in_act, statistics
 * in_mean / in_invstd): dx is then that unit's complete output gradient, and its BN-backward sums (mny_bn_bwd_reduce's: sum dz, sum dz*yhat)
 * are left in in_red as partial rows [mny_exdw_bwd_red_parts()][2][K] for mny_bn_bwd_finalize — no separate reduce pass over dx and x
 * (the project conv in front of the first expand unit, models/mobilenetv2.py:69-85).  Like mny_dw_bnbwd_red. */
int mny_exdw_bwd_red_parts(int N, int H, int W, int K, int C, int stride);
int mny_exdw_bwd_red(const float* gz, const float* z, const float* z_scale, const float* z_shift, int z_act, const float* z_coef,
                     const float* x, const float* in_scale, const float* in_shift, int in_act, const float* in_mean, const float* in_invstd,
                     const float* w_exp, const float* e_scale, const float* e_shift, const float* e_mean, const float* e_invstd,
                     const float* e_gamma, const float* w_dw, const float* addend, float* dx, float* dw_exp, float* dgamma_e, float* dbeta_e,
                     float* dw_dw, float* dw_ws, float* ws, float* in_red, int N, int H, int W, int K, int C, int stride, void* stream);

/* ---- stem + first depthwise unit, backward as one pass (csrc/stemdw.hip): the autograd of nn.Conv2d(3,32,3,2,1) + BN + ReLU6
 * (models/mobilenetv2.py:40,113) followed by the depthwise nn.Conv2d(32,32,3,1,1,groups=32) + BN + ReLU6 of the first InvertedResidual
 * (:65-67), given gd = dL/d act(d_scale d + d_shift) (the depthwise unit's output gradient), the depthwise unit's BN-backward
 * coefficients d_coef[3][32] (mny_bn_bwd_finalize), the raw outputs d (depthwise) and s (stem) with their BN coefficients, and the
 * NCHW fp32 image.  Replaces mny_dw_bnbwd_red + mny_bn_bwd_finalize + mny_stem_bnwgrad for that pair: the stem's output gradient is
 * never written (dW_stem = ca o (dz^T P) + cb o (W P^T P) + cc (x) colsum(P), P = the 27-value image patches; fp64 finalize).
 * Outputs: dw_stem[32,3,3,3], dgamma_s[32], dbeta_s[32], dw_dw[32,3,3] (or, dw_dw == NULL, partial rows
 * [mny_stemdw_bwd_parts()][32*9] left in dw_ws for mny_reduce_batch).  ws: mny_stemdw_bwd_ws_floats() floats; dw_ws:
 * mny_stemdw_bwd_parts() * 288 floats.  fp32 storage, Cout = 32, activations of the ReLU / ReLU6 / leaky family. */
int mny_stemdw_supported(int N, int H, int W, int Cout, int s_act, int d_act);
int mny_stemdw_bwd_parts(int N, int H, int W, int Cout);
size_t mny_stemdw_bwd_ws_floats(int N, int H, int W, int Cout);
int mny_stemdw_bwd(const float* gd, const float* d, const float* d_scale, const float* d_shift, int d_act, const float* d_coef,
                   const float* s, const float* s_scale, const float* s_shift, const float* s_mean, const float* s_invstd,
                   const float* s_gamma, int s_act, const float* x_nchw, const float* w_stem, const float* w_dw,
                   float* dw_stem, float* dgamma_s, float* dbeta_s, float* dw_dw, float* dw_ws, float* ws,
                   int N, int H, int W, int Cout, void* stream);

/* ---- project-conv unit, backward as one pass (csrc/pjbwd.hip): the autograd of the linear bottleneck nn.Conv2d(Ki,No,1) + BN that
 * closes an inverted-residual block (models/mobilenetv2.py:69-70,83-84), given g = dL/d(BN output) [M,No], the unit's raw conv output
 * y [M,No], its BN-backward coefficients coef[3][No] (mny_bn_bwd_finalize), and the raw output d [M,Ki] of the unit in front (the
 * depthwise unit; its view = d_scale / d_shift / d_act, its statistics d_mean / d_invstd), consumed only here.  Replaces
 * mny_bn_bwd_apply + mny_pw_dgrad_bnred + mny_pw_wgrad for that unit: gd[M,Ki] = dY W (the gradient wrt the activated d), the
 * BN-backward sums of the unit in front as partial rows red[mny_pj_bwd_parts()][2][Ki] (for mny_bn_bwd_finalize), and
 * dw[No,Ki] = dY^T act(BN(d)) (or, dw == NULL, partial rows [mny_pj_bwd_parts()][No*Ki] left in dw_ws).  d is read once, dY never
 * touches HBM.  No in {16,24,32}, Ki in {32,96,144,192}, fp32 storage. */
int mny_pj_bwd_supported(int64_t M, int Ki, int No, int d_act);
int mny_pj_bwd_parts(int64_t M, int Ki, int No);
int mny_pj_bwd(const float* g, const float* y, const float* coef, const float* d, const float* d_scale, const float* d_shift,
               const float* d_mean, const float* d_invstd, int d_act, const float* w, float* gd, float* dw, float* dw_ws, float* red,
               int64_t M, int Ki, int No, void* stream);
/* the same on bf16 storage (csrc/gate.hip, the wave-per-16-pixels matrix-core machinery of the gate unit): MobileNetV3's thin project
 * convs (models/mobilenetv3.py:57-58,69), (Ki, No) in {(16,16), (64,24), (72,24), (72,40), (120,40)}, any view activation but h-sigmoid;
 * the BN-backward sums of the unit in front are taken over the STORED (bf16) gd like mny_pw_dgrad_bnred_bf16's; dw's operands are the
 * bf16 values the forward GEMM multiplied. */
int mny_pj_bwd_supported_bf16(int64_t M, int Ki, int No, int d_act);
int mny_pj_bwd_parts_bf16(int64_t M, int Ki, int No);
int mny_pj_bwd_bf16(const void* g, const void* y, const float* coef, const void* d, const float* d_scale, const float* d_shift,
                    const float* d_mean, const float* d_invstd, int d_act, const float* w, void* gd, float* dw, float* dw_ws, float* red,
                    int64_t M, int Ki, int No, void* stream);

/* ---- MobileNetV3's per-pixel gate as one unit (csrc/gate.hip), bf16 storage: models/mobilenetv3.py:26-41 (SeModule whose avg_pool is
 * never called: the gate is per pixel) applied to the project conv's output (:69-71) —
 *     t = s3 * y3 + b3;  h = relu(BN1(W1 t));  gate = relu6(BN2(W2 h) + 3) / 6;  out = t * gate (+ view(add_x): the residual add of :72)
 * with the hidden tensors (and, backward, their gradients) never written.  Training-mode BatchNorm needs the batch statistics of W1 t
 * and of W2 h before they are used, so the forward is three streaming passes over y3 [M,C] with mny_bn_finalize in between:
 *   mny_gate_stats1_bf16 -> partial rows [mny_gate_parts(M)][2][R] of W1 t   (then mny_bn_finalize(..., R) -> sc1, sh1, mean1, invstd1)
 *   mny_gate_stats2_bf16 -> partial rows [mny_gate_parts(M)][2][C] of W2 h   (then mny_bn_finalize(..., C) -> sc2, sh2, mean2, invstd2)
 *   mny_gate_fwd_bf16    -> out [M,C]
 * and the backward, given dout = dL/d(out) [M,C] (the residual operand's gradient is dout itself), three more with
 * mny_bn_bwd_finalize in between:
 *   mny_gate_bwd1_bf16 -> BN2's backward sums, partial rows red2 [mny_gate_bwd_parts(M)][2][C]   (finalize -> dgamma2, dbeta2, coef2[3][C])
 *   mny_gate_bwd2_bf16 -> BN1's backward sums red1 [..][2][R] (finalize -> dgamma1, dbeta1, coef1[3][R]) and dW2 as partial
 *                         rows dw2_parts [mny_gate_bwd_parts(M)][C*R] (mny_reduce_batch)
 *   mny_gate_bwd3_bf16 -> dt [M,C] = dL/d(t) (both uses of t), dW1 as partial rows dw1_parts [..][R*C], and optionally
 *                         (red3 != NULL, mny_gate_bwd_red3_supported) the project unit's own BN-backward sums red3 [..][2][C] over
 *                         (dt, y3) — what a separate mny_bn_bwd_reduce pass would compute (mean3 / invstd3: its statistics).
 * wq: the two 1x1 conv weights (w1 [R,C], w2 [C,R], fp32 masters) cut into bf16 matrix-core operands, mny_gate_wq_bytes(C,R) bytes,
 * refreshed once per pass for all gates of a plan by mny_gate_cut_batch_bf16 (the gate's counterpart of the GEMM path's bf16 shadows).
 * (C, R) in {(40,10), (112,28), (160,40)} = MobileNetV3-Large's gates. */
typedef struct mny_gate_cut_job {
    const float* w1; /* [R][C] */
    const float* w2; /* [C][R] */
    void* wq;        /* mny_gate_wq_bytes(C, R) bytes */
    int32_t C, R;
} mny_gate_cut_job;
int mny_gate_supported(int64_t M, int C, int R);
int mny_gate_parts(int64_t M);
int mny_gate_bwd_parts(int64_t M);
int mny_gate_bwd_red3_supported(int C, int R);
size_t mny_gate_wq_bytes(int C, int R);
int mny_gate_cut_batch_bf16(const mny_gate_cut_job* jobs, int njobs, void* stream);
int mny_gate_stats1_bf16(const void* y3, const float* s3, const float* b3, const void* wq, float* stats, int64_t M, int C, int R,
                         void* stream);
int mny_gate_stats2_bf16(const void* y3, const float* s3, const float* b3, const void* wq, const float* sc1, const float* sh1,
                         float* stats, int64_t M, int C, int R, void* stream);
int mny_gate_fwd_bf16(const void* y3, const float* s3, const float* b3, const void* wq, const float* sc1, const float* sh1,
                      const float* sc2, const float* sh2, const void* add_x, const float* add_scale, const float* add_shift,
                      int add_act, void* out, int64_t M, int C, int R, void* stream);
int mny_gate_bwd1_bf16(const void* y3, const float* s3, const float* b3, const void* dout, const void* wq, const float* sc1,
                       const float* sh1, const float* sc2, const float* sh2, const float* mean2, const float* invstd2, float* red2,
                       int64_t M, int C, int R, void* stream);
int mny_gate_bwd2_bf16(const void* y3, const float* s3, const float* b3, const void* dout, const void* wq, const float* sc1,
                       const float* sh1, const float* mean1, const float* invstd1, const float* sc2, const float* sh2,
                       const float* coef2, float* red1, float* dw2_parts, int64_t M, int C, int R, void* stream);
int mny_gate_bwd3_bf16(const void* y3, const float* s3, const float* b3, const void* dout, const void* wq, const float* sc1,
                       const float* sh1, const float* sc2, const float* sh2, const float* coef2, const float* coef1,
                       const float* mean3, const float* invstd3, void* dt, float* dw1_parts, float* red3, int64_t M, int C, int R,
                       void* stream);

/* ---- Anchor fitting (csrc/anchors.hip): the anchors of config["yolo"]["anchors"] fitted to a label set on the device — k-means under
 * the shape IoU, the fitness of many candidate sets in one launch, a mutation search, and a census of what mny_yolo_loss's target
 * assignment will do with a set of anchors.  The reference has no counterpart: its anchors arrive ready-made in the config.  This text
 * is the specification (restated in numpy by tests/anchor_ref.py); k-means and the search are not pinned against any third-party
 * "autoanchor".  The census is pinned: it reproduces the positive count of mny_yolo_loss, and through the oracle get_target's.
 *
 * Shapes are wh[N,2] fp32 on the device, (w, h) in pixels, 16-byte aligned.
 * Valid boxes.  A box is valid iff 2^-20 <= w <= 65536 and 2^-20 <= h <= 65536 (NaN fails the test).  Invalid boxes take part in
 *   nothing and are counted in `skipped`.  Limits: 1 <= k <= 32, 1 <= N <= 2^22, 1 <= P <= 256; anything else is MNY_EINVAL with a
 *   message and without a launch.  Centres, anchors and candidates are expected positive and finite (an IoU that is NaN never wins).
 * Shape IoU.  inter = min(w,aw) * min(h,ah);  v = inter / ((w*h + aw*ah) - inter), every operation fp32 round-to-nearest in this
 *   order, no contraction: find_jaccard_overlap (utils/iou.py:32-49) on [0,0,w,h] and [0,0,aw,ah].  best = the lowest index with the
 *   largest v (strict >, starting from -inf at index 0).
 * Fixed point.  Every sum that crosses lanes or workgroups is an integer, so no result depends on the launch order (no float atomics):
 *   q(x) = llrint((double)x * 2^24) for shapes, qi(v) = llrint((double)v * 2^32) for IoUs (round to nearest even).
 * k-means step.  (1) label every valid box with `best` against the current centres; (2) per centre S_w, S_h = int64 sums of q over
 *   its boxes and n = their count; (3) a centre with n > 0 becomes (float)(((double)S / (double)n) * 2^-24) per coordinate; (4) a
 *   centre with n == 0 keeps its value.  The run has converged at the first step that changes no bit of any centre; later steps are
 *   the identity (the library skips them on a device flag).
 *   mny_anchor_kmeans: centres[k,2] holds the initial centres and receives the result; max_iter (0..100000) steps are queued with no
 *   host synchronisation, then a final pass writes labels[N] (int32 `best`, -1 for a skipped box) and, unless NULL, best_iou[N] (0
 *   for a skipped box).  state = int64[4] on the device: {steps run up to and including the first that changed nothing (max_iter when
 *   none did), converged 0/1, skipped, 0}.
 * Fitness of P candidate sets cand[P,k,2] in one launch (mny_anchor_fitness): F[p] = sum of qi(best_v) over the valid boxes with
 *   best_v > thr, R[p] = their count; thr is fp32 and thr = 0 gives the plain mean best IoU.  out = int64 [P][2] = (F, R); valid[1] =
 *   the number of valid boxes.  mean best IoU = F * 2^-32 / valid, recall = R / valid.
 * Evolution (mny_anchor_evolve): factors[G,P,k,2] fp32 on the device.  The parent starts as anchors_in[k,2].  In generation g candidate
 *   0 is the parent verbatim and candidate p >= 1 is max(parent * factors[g,p], min_size) elementwise in fp32 (fmaxf); the candidate
 *   with the largest F becomes the parent, ties to the lowest p, so F never decreases.  history = int64 [G][2] = (winning F, its p);
 *   anchors_out[k,2] = the last parent (may alias anchors_in).  No host synchronisation inside.  How the factors are drawn is not part
 *   of the ABI (anchors.draw_factors).  2^-20 <= min_size <= 65536.
 * Census (mny_anchor_census): what mny_yolo_loss will do with these anchors.  targets[T,5] packed in the loss's layout (label, cx, cy,
 *   w, h, relative to the image; 0 <= T <= 2^24), anchors_all[n,2] already divided by the image size (n <= 64), H <= 4 heads with
 *   mask[H][A] (A <= 16) and grids[H] — these two are HOST arrays — and iou_thresh.  For every target, exactly as yolo_assign_kernel
 *   (models/yolo_loss.py:127-146): best_n over all n anchors by the box IoU with the first maximum winning and a NaN counting as the
 *   maximum; gi = (int)(cx * g), gj = (int)(cy * g) (truncation), the target is outside head h unless 0 <= gi, gj < g; otherwise
 *   anchor slot a of head h is hit iff mask[h][a] == best_n or iou > iou_thresh.  out = int64 [n + H*A + 1 + H] =
 *   best[n] (histogram of best_n over all targets) | pos[H][A] (hits: sum over a = the loss's count) | orphans (targets with no hit
 *   in any head) | outside[H].
 * ws: mny_anchor_ws_bytes(k, P) bytes, 16-byte aligned, for mny_anchor_kmeans (P = 1) and mny_anchor_evolve; the caller allocates
 * everything and nothing is retained between calls. */
size_t mny_anchor_ws_bytes(int k, int P);
int mny_anchor_kmeans(const float* wh, int64_t N, float* centres, int k, int max_iter, int32_t* labels, float* best_iou, int64_t* state,
                      void* ws, void* stream);
int mny_anchor_fitness(const float* wh, int64_t N, const float* cand, int P, int k, float thr, int64_t* out, int64_t* valid, void* stream);
int mny_anchor_evolve(const float* wh, int64_t N, const float* anchors_in, int k, const float* factors, int G, int P, float thr,
                      float min_size, float* anchors_out, int64_t* history, void* ws, void* stream);
int mny_anchor_census(const float* targets, int64_t T, const float* anchors_all, int n, const int32_t* mask, const int32_t* grids, int H,
                      int A, float iou_thresh, int64_t* out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MNYOLO_H */
