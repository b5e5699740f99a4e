/*
 * abr_iod_hip.h -- C ABI of libabr_iod_hip.so (hand-written HIP for gfx950 / MI355X).
 *
 * Drop-in boundary for the Faster R-CNN + ARD training hot path of YuyangSunshine/ABR_IOD.
 * The reference crosses into native code through the pybind11 module `maskrcnn_benchmark._C`
 * (maskrcnn_benchmark/csrc/vision.cpp:9-25); everything else on the path is ATen (cuDNN/cuBLAS/
 * elementwise).  This library exports BOTH: section 1 mirrors `_C` one-to-one, sections 2-5 replace
 * the ATen work the path does per step.  Citations are file:line under /root/reference/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; no torch types anywhere
 *   - outputs are caller-allocated (the Python host allocates them with torch so allocator / stream
 *     semantics match the reference's at::empty, csrc/cuda/ROIAlign_cuda.cu:271,316)
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and the call returns
 *     without synchronising (reference: at::cuda::getCurrentCUDAStream(), ROIAlign_cuda.cu:273)
 *   - return 0 on success, <0 on error (ABR_E_*); abr_last_error() gives the message (the reference
 *     raises C++ exceptions -> Python RuntimeError; the Python host re-raises RuntimeError)
 *   - empty inputs are legal and return 0 without launching (ROIAlign_cuda.cu:278-281, nms.h:15-16)
 *   - layouts: ABR_NCHW is the reference's tensor layout (drop-in); ABR_NHWC is the library's native
 *     layout (channel-contiguous => 4 KB coalesced rows at C=1024)
 */
#ifndef ABR_IOD_HIP_H
#define ABR_IOD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABR_OK 0
#define ABR_E_INVALID (-1) /* bad argument (AT_ASSERTM in the reference) */
#define ABR_E_LAUNCH (-2)  /* hipGetLastError() != success after a launch (THCudaCheck) */
#define ABR_E_WORKSPACE (-3)

#define ABR_NCHW 0
#define ABR_NHWC 1

const char* abr_last_error(void);
int abr_version(void);
/* device properties the host side needs for grid sizing: out[0]=CU count, out[1]=LDS bytes/CU, out[2]=wave size */
int abr_device_info(int32_t* out_host);

/* Per-launch timing of the conv kernels with HIP events on the launch stream (bench.py's roofline leg; off by default).
 * abr_prof_end: out[id*6+{0,1,2}] = {launches, total ms, total flops} of the launches that had the device to themselves,
 * out[id*6+{3,4,5}] = the same for launches made while abr_prof_mark_overlap(1) was in force (the host runs weight-gradient
 * kernels on a second stream next to the dgrad chain: those launches share CUs and their event-bracketed duration is not a
 * property of the kernel).  id = 0 igemm 128x128, 1 igemm 128x64, 2 igemm 64x64, 3 igemm small-C (stem), 4 wgrad, 5/6 ROIAlign
 * fwd/bwd, 7 igemm bf16 (one-product instances of the weights-direct kernel), 8 wgrad bf16 / bf16x6, 9 / 10 / 11 the bf16x6 implicit GEMM's 128x128 / 128x64 / 64x64 tile instances, 12 / 13 / 14 the same tiles of its weights-direct form.  Synchronises on the recorded events and stops profiling. */
int abr_prof_begin(void);
int abr_prof_mark_overlap(int on);
/* Order everything queued on `waiter` from now on behind everything queued on `signaller` so far (an event recorded on `signaller`, waited for by
 * `waiter`: torch's side.wait_stream(cur) in ONE call of ~2 us instead of ~15 us of Python -- the training step orders ~60 weight gradients so). */
int abr_stream_wait_stream(void* waiter, void* signaller);
/* bit id set = time that kernel (default all); every_nth = n > 1: bracket launch i of a kernel in step s iff (i + s) % n == 0 (an
 * event pair costs a ~6 us pipeline bubble per launch).  The caller marks step boundaries with abr_prof_step_begin(); over n
 * consecutive steps every launch position of the step's fixed launch sequence is sampled exactly once. */
int abr_prof_set_mask(uint32_t id_mask, int every_nth);
int abr_prof_step_begin(void);
int abr_prof_end(double* out_host, int n_ids);
/* out[id*2+{0,1}] = {launches, total flops} of EVERY launch of kernel id since abr_prof_begin, event-bracketed or not (call before
 * abr_prof_end or after: the totals survive until the next abr_prof_begin) */
int abr_prof_totals(double* out_host, int n_ids);
/* out[id] = ALGORITHMIC HBM bytes (every operand and the output once, + a fused residual / mask read) of every launch of kernel id since
 * abr_prof_begin: next to the PMC traffic of the same kernel it says how much of the traffic is re-reads (bench.py: roofline.traffic_algorithmic) */
int abr_prof_bytes(double* out_host, int n_ids);
/* out[id*2 + {0,1}] = {shader cycles (s_memtime), milliseconds (s_memrealtime)} that workgroup 0 of the sampled self-stamping launches of kernel
   id ran, summed by the last abr_prof_end: cycles / ms / 1e6 = the clock in GHz the chip sustained under that kernel (it clocks to its power budget) */
int abr_prof_clocks(double* out_host, int n_ids);
/* median duration (ms) of an event pair around an EMPTY kernel on a busy stream: the share of an event-bracketed duration that is
 * dispatch gap, not kernel; bench.py subtracts it from its live per-launch durations (synchronises the stream) */
int abr_prof_event_overhead_ms(double* out_host, void* stream);

/* Range guard of the bf16x6 arithmetic (abr_conv_desc::math == ABR_MATH_BF16X6).  The three-way bf16 split x = x0 + x1 + x2 is
 * EXACT -- and the contraction then meets the fp32 error bound -- for operands that are zero or have 2^-110 <= |x| < 2^128 (finite);
 * below 2^-110 the low planes leave bf16's normal range and precision decays towards bf16's, and an inf operand yields NaN
 * (inf - inf in the split) where an fp32 multiply-add chain yields inf.  Every bf16x6 kernel inspects each operand element once per
 * GEMM and ORs ABR_X6_FLAG_* into a device word; abr_x6_range_flags copies it to *out_host (synchronising `stream`) and, if `reset`,
 * clears it.  A caller that needs the fp32 result for out-of-domain data re-runs the operation with ABR_MATH_F32 when a flag is up
 * (the Python host does: ops.x6_range_flags, engine/trainer.py). */
#define ABR_X6_FLAG_TINY 1u
#define ABR_X6_FLAG_NONFINITE 2u
/* f16x3 arithmetic (ABR_MATH_F16X3), same flag word: STALE = an amax word did not carry the epoch the caller named (a caller bug: the kernel
 * then ran with scale 1); a non-finite amax raises ABR_X6_FLAG_NONFINITE.  Operand elements more than 18 binades below their tensor's amax
 * (they keep an ABSOLUTE accuracy of 2^-40 amax instead of 2^-22 relative) are ordinary and are COUNTED, not flagged: abr_h3_range_stats. */
#define ABR_H3_FLAG_STALE 8u
int abr_x6_range_flags(uint32_t* out_host, int reset, void* stream);
/* the same word copied to PINNED host memory on `stream` without synchronising (the trainer polls it one step later) */
int abr_x6_range_flags_async(uint32_t* out_pinned_host, void* stream);
/* the same word copied to DEVICE memory on `stream` (data-parallel training MAX-reduces it over the ranks with RCCL before reading it,
 * so that every rank leaves the bf16x6 arithmetic at the same step: engine/trainer.py::_x6_guard) */
int abr_x6_range_flags_to_device(uint32_t* out_device, void* stream);

/* =====================================================================================================
 * 1. maskrcnn_benchmark._C  (csrc/vision.cpp:10-16)
 * ===================================================================================================== */

/* _C.roi_align_forward(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio)
 *   csrc/ROIAlign.h:11-25 -> csrc/cuda/ROIAlign_cuda.cu:65-122,258-300 / csrc/cpu/ROIAlign_cpu.cpp:113-256
 * feat [B,C,H,W] (NCHW) or [B,H,W,C] (NHWC); rois [K,5] = (batch_idx,x1,y1,x2,y2) fp32;
 * out  [K,C,PH,PW] (NCHW) or [K,PHo,PWo,C] (NHWC) where PHo=ceil(PH/bin_step).
 * bin_step: 1 = every bin (reference behaviour).  2 = only bins with even (ph,pw): what a following
 *   stride-2 1x1 conv (ResNetHead.layer4.0, modeling/backbone/resnet.py:278) actually reads; NHWC only. */
int abr_roi_align_forward(const float* feat, const float* rois, int K, int B, int C, int H, int W,
                          float spatial_scale, int PH, int PW, int sampling_ratio, int bin_step,
                          int layout, float* out, void* stream);

/* _C.roi_align_backward(grad, rois, spatial_scale, ph, pw, B, C, H, W, sampling_ratio)
 *   csrc/ROIAlign.h:27-45 -> csrc/cuda/ROIAlign_cuda.cu:178-254,304-346 (CPU: "Not implemented").
 * grad_feat is zero-filled by the callee unless accumulate!=0 (reference: at::zeros, :316). */
int abr_roi_align_backward(const float* grad, const float* rois, int K, int B, int C, int H, int W,
                           float spatial_scale, int PH, int PW, int sampling_ratio, int bin_step,
                           int layout, int accumulate, float* grad_feat, void* stream);

/* The float64 instantiations of the reference's dispatch (AT_DISPATCH_FLOATING_TYPES: csrc/cuda/ROIAlign_cuda.cu:283,329, csrc/cpu/ROIAlign_cpu.cpp:242):
 * NCHW tensors, every T of the reference's templates = double.  grad_feat is zero-filled by the callee (at::zeros, :316). */
int abr_roi_align_forward_f64(const double* feat, const double* rois, int K, int B, int C, int H, int W, double spatial_scale, int PH, int PW,
                              int sampling_ratio, double* out, void* stream);
int abr_roi_align_backward_f64(const double* grad, const double* rois, int K, int B, int C, int H, int W, double spatial_scale, int PH, int PW,
                               int sampling_ratio, double* grad_feat, void* stream);

/* Same result as abr_roi_align_backward(layout=ABR_NHWC) without atomics: every feature pixel gathers from the RoIs that
 * cover it (two kernels: per-RoI separable weight tables, then one coalesced write per dFeat element, deterministic order).
 * workspace: abr_roi_align_backward_ws_bytes(...) bytes.  This is the form the training step uses. */
int64_t abr_roi_align_backward_ws_bytes(int K, int B, int H, int W, int PH, int PW, int bin_step);
int abr_roi_align_backward_gather(const float* grad, const float* rois, int K, int B, int C, int H, int W,
                                  float spatial_scale, int PH, int PW, int sampling_ratio, int bin_step, int accumulate,
                                  float* grad_feat, void* workspace, int64_t workspace_bytes, void* stream);

/* Integer tap table of the forward kernel's OWN indexing code (parity instrument, not on the hot path):
 * idx [K,PH*PW,max_s,4] int32 flat y*W+x (-1 = sample rejected, -2 = unused slot), grid [K,2]. */
int abr_roi_align_taps(const float* rois, int K, int H, int W, float spatial_scale, int PH, int PW,
                       int sampling_ratio, int max_s, int32_t* idx, int32_t* grid, void* stream);

/* Pooling over a feature pyramid: modeling/poolers.py (LevelMapper :11-42, Pooler.forward :80-105), which is Python over _C.roi_align_* in the
 * reference (per level a nonzero, a row gather, one ROIAlign launch, an indexed write into zeros).  Here one launch each way.
 *
 * Level of a row, in fp32 with the reference's operations in its order (IEEE sqrt and division, no contraction):
 *   area = (x2 - x1 + 1) * (y2 - y1 + 1);  t = floor(canonical_level + log2(sqrt(area) / canonical_scale + eps));
 *   level = (int)clamp(t, k_min, k_max) - (int)k_min.
 * A negative or NaN area makes t NaN: that row has NO level, reported as -1; its output row is all zero and it adds nothing to any gradient
 * (in the reference it matches no level and its row of the zero-filled result stays).  area == 0 is an ordinary row (it clamps to k_min).
 * Once the level is chosen a row is pooled exactly as abr_roi_align_forward(layout = ABR_NHWC, bin_step = 1) pools it on that level's map
 * with that level's scale: same taps, weights, association order and /count, so the same bits.
 *
 * 1 <= L <= ABR_MAX_PYRAMID_LEVELS; (int)k_max - (int)k_min < L; H[l], W[l] >= 1 with no relation between the levels; any C >= 1;
 * K * PH * PW * C and every B * H[l] * W[l] * C must fit int32.  feats / grad_feats, H, W and scales are HOST arrays of L entries that the call
 * copies into the kernel's arguments: there is no device-side table and nothing to keep alive after the call returns.
 * NOT provided for pyramids: an atomic-free gather backward like abr_roi_align_backward_gather, bin_step = 2, NCHW memory, float64. */
#define ABR_MAX_PYRAMID_LEVELS 8

/* rois [K,5] -> levels [K] int32 in 0 .. (int)k_max - (int)k_min, or -1 for a row without a level */
int abr_fpn_levels(const float* rois, int K, float k_min, float k_max, float canonical_scale, float canonical_level, float eps,
                   int32_t* levels, void* stream);

/* feats_host[l] = device pointer of level l's map [B,H[l],W[l],C] (NHWC fp32); out [K,PH,PW,C]; levels_out [K] int32 or NULL.
 * K == 0 launches nothing. */
int abr_roi_align_pyramid_forward(const float* const* feats_host, const int* H_host, const int* W_host, const float* scales_host, int L,
                                  const float* rois, int K, int B, int C, int PH, int PW, int sampling_ratio,
                                  float k_min, float k_max, float canonical_scale, float canonical_level, float eps,
                                  float* out, int32_t* levels_out, void* stream);

/* grad [K,PH,PW,C] -> grad_feats_host[l] [B,H[l],W[l],C]: every element of every level, reached by a RoI or not, is written (the sum, or
 * 0) unless accumulate != 0, then added to (also when K == 0).  One launch over the RoIs scatters each into its level with hardware atomics;
 * each RoI's addend is computed in fp32 as abr_roi_align_backward computes it, but the atomics add into zeroed float64 scratch that the library
 * owns (8 bytes per gradient element of all levels, per stream) and a second launch rounds every sum to fp32 once: an element that hundreds of
 * RoIs reach is then not a float32 sum in arrival order.  The order of the adds still varies from run to run, and with it, rarely, a last bit.
 * ABR_E_WORKSPACE when the scratch cannot be allocated. */
int abr_roi_align_pyramid_backward(const float* grad, const float* rois, int K, int B, int C, const int* H_host, const int* W_host,
                                   const float* scales_host, int L, int PH, int PW, int sampling_ratio,
                                   float k_min, float k_max, float canonical_scale, float canonical_level, float eps,
                                   int accumulate, float* const* grad_feats_host, void* stream);

/* The indexed forms: pool (scatter) only the rows of the table that a device list names, one launch each way, no gathered copy of the table.
 * rois [K,5]; rows [P] int64 on the device; out / grad [P,PH,PW,C]; levels_out [P] int32 or NULL.  out[p] has exactly the bits
 * abr_roi_align_pyramid_forward gives row rows[p]; an entry < 0 or >= K is padding: its table row is never read, out[p] is all zero and its
 * level -1; the backward adds nothing for it and does not read grad[p] (which may hold NaN).  The grid is over P; P * PH * PW * C must fit
 * int32.  Scratch, rounding and `accumulate` as in abr_roi_align_pyramid_backward; P == 0 behaves as K == 0 does there (rows may be NULL). */
int abr_roi_align_pyramid_rows_forward(const float* const* feats_host, const int* H_host, const int* W_host, const float* scales_host, int L,
                                       const float* rois, int K, const int64_t* rows, int P, int B, int C, int PH, int PW, int sampling_ratio,
                                       float k_min, float k_max, float canonical_scale, float canonical_level, float eps,
                                       float* out, int32_t* levels_out, void* stream);
int abr_roi_align_pyramid_rows_backward(const float* grad, const float* rois, const int64_t* rows, int P, int K, int B, int C, const int* H_host,
                                        const int* W_host, const float* scales_host, int L, int PH, int PW, int sampling_ratio,
                                        float k_min, float k_max, float canonical_scale, float canonical_level, float eps,
                                        int accumulate, float* const* grad_feats_host, void* stream);

/* The top-down pathway of a feature pyramid network (modeling/backbone/fpn.py:47-70) and LastLevelMaxPool (:90-92), csrc/fpn.hip.
 * All maps are NHWC fp32, contiguous, 16-byte aligned, C % 4 == 0; level 0 is the finest, H[l] == 2 H[l+1] and W[l] == 2 W[l+1];
 * 1 <= L <= ABR_MAX_PYRAMID_LEVELS; B * H[0] * W[0] * C / 4 must fit int32.  The *_host arguments are HOST arrays of L entries copied into the
 * kernel's arguments.  Every refusal (negative status, abr_last_error names the argument) comes before any launch.  No atomics: every output
 * element has one owner and its additions a fixed order, so results reproduce bit for bit.
 *
 * Forward, one launch: inner_host[l], l < L-1, receives inner_l(y,x) = lat_l(y,x) + inner_{l+1}(y>>1, x>>1) with inner_{L-1} = lat_{L-1};
 * each element is evaluated from the top down (t = lat_{L-1}; t = lat_{L-2} + t; ... ; t = lat_l + t), only fp32 adds: bit-equal to the
 * level-by-level lateral + F.interpolate(last_inner, scale_factor=2, mode="nearest").  inner_host[L-1] is never read or written (the top
 * level IS its lateral); inner_host[l] may not alias a lateral.  L == 1 launches nothing. */
int abr_fpn_topdown_forward(const float* const* lat_host, float* const* inner_host, const int* H_host, const int* W_host, int L, int B, int C,
                            void* stream);
/* Its adjoint, one launch: g_host[l] = the gradient arriving at inner_l (NULL for l >= 1: none, a zero that is not added; g_host[0] is required),
 * d_lat_host[l] receives T_l, T_0 = g_0,
 *   T_l(y,x) = g_l(y,x) + ((T_{l-1}(2y,2x) + T_{l-1}(2y,2x+1)) + (T_{l-1}(2y+1,2x) + T_{l-1}(2y+1,2x+1)))      (without g_l: the bracket alone)
 * in exactly this order of fp32 additions.  One thread per (image, coarsest pixel, 4 channels) folds its descendants from the finest level
 * up: every g is read once, every d_lat written once.  d_lat_host[l] == g_host[l] is allowed (T_l written over g_l; nothing is copied for
 * level 0 then). */
int abr_fpn_topdown_backward(const float* const* g_host, float* const* d_lat_host, const int* H_host, const int* W_host, int L, int B, int C,
                             void* stream);
/* LastLevelMaxPool = F.max_pool2d(x, 1, 2, 0): out [B,Ho,Wo,C] (y,x) = x [B,H,W,C] (2y,2x), Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1 */
int abr_fpn_subsample2_forward(const float* x, int B, int H, int W, int C, float* out, void* stream);
/* g_x [B,H,W,C] written whole: g_in (NULL: zero) + g_out [B,Ho,Wo,C] scattered to the even pixels; g_x == g_in is allowed */
int abr_fpn_subsample2_backward(const float* g_out, const float* g_in, int B, int H, int W, int C, float* g_x, void* stream);

/* _C.roi_pool_forward(input, rois, spatial_scale, pooled_h, pooled_w) -> (output, argmax)
 *   csrc/ROIPool.h:10-24 -> csrc/cuda/ROIPool_cuda.cu:16-77,110-150 (there is no CPU implementation).
 * feat [B,C,H,W] (NCHW) or [B,H,W,C] (NHWC); rois [K,5]; out and argmax [K,C,PH,PW] (NCHW) or [K,PH,PW,C] (NHWC).
 * argmax is the flat pixel h*W+w of the bin's first maximum in BOTH layouts, -1 for an empty bin (value 0) and for a bin without a
 * value above -FLT_MAX (value -FLT_MAX).  Bin borders are floor / ceil of fp32 products, as the reference computes them.
 * Error when K*C*PH*PW or B*C*H*W does not fit int32; no launch when K == 0. */
int abr_roi_pool_forward(const float* feat, const float* rois, int K, int B, int C, int H, int W, float spatial_scale, int PH, int PW,
                         int layout, float* out, int32_t* argmax, void* stream);

/* _C.roi_pool_backward(grad, input, rois, argmax, spatial_scale, ph, pw, B, C, H, W)   csrc/ROIPool.h:26-47 -> ROIPool_cuda.cu:79-108,153-195
 * grad_feat[b, argmax] += grad wherever argmax != -1 (fp32 atomics: the order of the adds varies from run to run).
 * grad_feat is zero-filled by the callee unless accumulate != 0 (reference: at::zeros, :166). */
int abr_roi_pool_backward(const float* grad, const float* rois, const int32_t* argmax, int K, int B, int C, int H, int W, int PH, int PW,
                          int layout, int accumulate, float* grad_feat, void* stream);

/* The float64 instantiations of the reference's dispatch (AT_DISPATCH_FLOATING_TYPES, ROIPool_cuda.cu:134,177): NCHW tensors, the
 * geometry in double.  grad_feat is zero-filled by the callee. */
int abr_roi_pool_forward_f64(const double* feat, const double* rois, int K, int B, int C, int H, int W, double spatial_scale, int PH, int PW,
                             double* out, int32_t* argmax, void* stream);
int abr_roi_pool_backward_f64(const double* grad, const double* rois, const int32_t* argmax, int K, int B, int C, int H, int W, int PH, int PW,
                              double* grad_feat, void* stream);

/* _C.deform_psroi_pooling_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim, group_size, pooled_size,
 *                                 part_size, sample_per_part, trans_std)
 *   csrc/deform_pool.h:11-40 -> csrc/cuda/deform_pool_cuda.cu:33-82 -> deform_pool_kernel_cuda.cu:54-141; float32.
 * feat [B,C,H,W] / [B,H,W,C] with C >= OD*G*G; rois [K,5]; trans [K,2*num_classes,part,part] in both layouts, NULL = no_trans;
 * out and top_count [K,OD,P,P] (NCHW) or [K,P,P,OD] (NHWC).
 * mask_logits [K,P,P] (optional, beyond the reference): out is multiplied by sigmoid(mask_logits) of its bin -- the product that
 * ModulatedDeformRoIPoolingPack (layers/dcn/deform_pool_module.py:145-150) forms with torch ops. */
int abr_deform_psroi_forward(const float* feat, const float* rois, const float* trans, const float* mask_logits, int K, int B, int C, int H,
                             int W, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                             float trans_std, int num_classes, int layout, float* out, float* top_count, void* stream);

/* _C.deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad, no_trans, ...)
 *   csrc/deform_pool.h:43-70 -> deform_pool_kernel_cuda.cu:143-264.
 * grad_feat: fp32 atomics ADDED into the caller's buffer (the reference accumulates into input_grad too).
 * grad_trans [K,2*num_classes,part,part] (NULL exactly when trans is) and grad_mask_logits [K,P,P] (NULL exactly when mask_logits is)
 * are WRITTEN, every element by its one owner in a fixed order: no atomics, bit-reproducible. */
int abr_deform_psroi_backward(const float* out_grad, const float* feat, const float* rois, const float* trans, const float* mask_logits,
                              const float* top_count, int K, int B, int C, int H, int W, float spatial_scale, int output_dim, int group_size,
                              int pooled_size, int part_size, int sample_per_part, float trans_std, int num_classes, int layout,
                              float* grad_feat, float* grad_trans, float* grad_mask_logits, void* stream);

/* _C.nms(dets, scores, threshold)   csrc/nms.h:10-27 -> csrc/cpu/nms_cpu.cpp:5-75 / csrc/cuda/nms.cu:70-131
 * Batched, boxes already sorted by descending score (the reference sorts first: nms_cpu.cpp:24, nms.cu:73).
 *   boxes   [N, n_max, 4] xyxy fp32, image i uses its first counts[i] rows
 *   strict_gt : 0 -> suppress when IoU >= thr (CPU rule, nms_cpu.cpp:60; the canonical one here)
 *               1 -> suppress when IoU >  thr (CUDA rule, nms.cu:60)
 *   keep    [N, max_keep] int32 : positions (in sorted order) of survivors, ascending; n_keep [N] int32
 *   The greedy sweep runs ON DEVICE (no 18 MB D2H + host loop as nms.cu:99-123) and stops at max_keep.
 *   workspace: abr_nms_workspace_bytes(N, n_max) bytes. */
int64_t abr_nms_workspace_bytes(int N, int n_max);
int abr_nms_sorted_batched(const float* boxes, const int32_t* counts, int N, int n_max, float thr,
                           int strict_gt, int max_keep, int32_t* keep, int32_t* n_keep,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* _C.nms on UNSORTED boxes in one call (round 5; abr_iod_amd/_C.py::nms): descending stable score sort (abr_sort_scores_desc: the proposal
 * ranking's own kernels on order-preserving keys), greedy suppression as above, survivors' ORIGINAL indices in ascending order (nms.cu:127-130).
 *   dets [n,4] xyxy fp32 (16-byte aligned), scores [n] fp32, n <= abr_sort_scores_max_n() (15360); keep_out [n] int64, *n_keep_out int32 (device);
 *   workspace: abr_nms_unsorted_workspace_bytes(n) bytes. */
int64_t abr_nms_unsorted_workspace_bytes(int n);
int abr_nms(const float* dets, const float* scores, int n, float thr, int strict_gt, int64_t* keep_out, int32_t* n_keep_out, void* workspace,
            int64_t workspace_bytes, void* stream);
/* order[i] = index of the i-th largest score (ties: ascending index -- torch.sort(descending=True, stable=True)); any finite fp32 */
int64_t abr_sort_scores_max_n(void);
int abr_sort_scores_desc(const float* scores, int n, int64_t* order, void* stream);

/* _C.sigmoid_focalloss_forward / _backward   csrc/SigmoidFocalLoss.h:10-41 -> csrc/cuda/SigmoidFocalLoss_cuda.cu:20-101
 * logits [N,C] fp32, targets [N] int32 (0 = background, -1 = ignore, c>=1 = class c), losses/d_logits [N,C]. */
int abr_sigmoid_focal_forward(const float* logits, const int32_t* targets, int N, int C, float gamma,
                              float alpha, float* losses, void* stream);
int abr_sigmoid_focal_backward(const float* logits, const int32_t* targets, const float* d_losses, int N,
                               int C, float gamma, float alpha, float* d_logits, void* stream);
/* the float64 instantiations (AT_DISPATCH_FLOATING_TYPES, SigmoidFocalLoss_cuda.cu:128,172): T = double with the template's own float gamma /
 * alpha and expf / powf / logf calls */
int abr_sigmoid_focal_forward_f64(const double* logits, const int32_t* targets, int N, int C, float gamma, float alpha, double* losses, void* stream);
int abr_sigmoid_focal_backward_f64(const double* logits, const int32_t* targets, const double* d_losses, int N, int C, float gamma, float alpha,
                                   double* d_logits, void* stream);

/* =====================================================================================================
 * 2. Distillation + detector losses (ATen elementwise/reduction chains in the reference)
 *    Every loss kernel writes its scalar to loss_out[0] (device, loss_out must hold >= 4 floats) and, when grad pointers are non-NULL,
 *    the gradient for upstream-gradient `gscale` in the same launch sequence.
 * ===================================================================================================== */

/* calculate_attentive_roi_feature_distillation(f_map_s=SOURCE, f_map_t=TARGET, gamma)
 *   maskrcnn_benchmark/distillation/distillation.py:86-130, call site tools/train_incremental.py:115.
 * f_src,f_tgt [N,HW,C] (NHWC) or [N,C,HW] (NCHW).
 * coef [N,2,HW] fp32 scratch: a_src and dPad/dm_tgt per position, written by forward, read by backward.
 * loss_out[0] = afd + gamma*pad ; loss_out[1] = afd ; loss_out[2] = pad. */
int abr_ard_forward(const float* f_src, const float* f_tgt, int N, int C, int HW, float gamma, int layout,
                    float* coef, float* loss_out, void* stream);
/* grad_tgt = gscale * d(afd+gamma*pad)/d f_tgt ; gscale_dev (optional device scalar) multiplies gscale. */
int abr_ard_backward(const float* f_src, const float* f_tgt, const float* coef, int N, int C, int HW,
                     float gamma, int layout, float gscale, const float* gscale_dev, float* grad_tgt,
                     void* stream);

/* smooth_l1_loss(input, target, beta, size_average)   maskrcnn_benchmark/layers/smooth_l1_loss.py:6-17
 * Optional row gather: when rows!=NULL only rows[i] (int64) of x/t take part and, per row, the 4 columns
 * starting at col0[i] of x (box_head/loss.py:166-172 advanced indexing); x_cols = row length of x.
 * loss_out[0] = sum * scale.  grad (optional, same shape as x, must be pre-zeroed when rows!=NULL). */
int abr_smooth_l1(const float* x, const float* t, int64_t n, float beta, float scale, float* loss_out,
                  float gscale, float* grad, void* stream);
int abr_smooth_l1_rows(const float* x, int x_cols, const float* t, const int64_t* rows, const int64_t* col0,
                       const int64_t* trows /* rows of t, NULL = rows */, int n_rows, float beta, float scale,
                       const float* denom_dev /* optional device scalar: scale /= max(*denom_dev,1); rows < 0 are skipped */,
                       float* loss_out, float gscale, float* grad, void* stream);

/* FastRCNNLossComputation classification term   modeling/roi_heads/box_head/loss.py:151-162
 *   inclusive != 0 : "Inclusive Classification Loss" (dist_type=='id'), n_old = number of old classes
 *   else           : F.cross_entropy.   labels int64 [n]; label<0 rows are ignored as F.nll_loss does (-100)
 * loss_out[0] = mean over counted rows.  d_logits optional [n,K]. */
int abr_softmax_ce(const float* logits, int ld_logits /* row pitch, <=0: K */, const int64_t* labels, int n, int K,
                   int inclusive, int n_old, float* loss_out, float gscale, float* d_logits, int ld_dlogits,
                   void* stream);

/* calculate_feature_distillation_loss(..., loss='normalized_filtered_l1')  distillation.py:133-161 (ablation DIST.FEAT='std'), one
 * feature level: loss = mean(max((s - mean s) - (t - mean t), 0)) over all n elements (any memory order).  stats3: 3-float scratch.
 * d_tgt (optional, n floats) = gscale * dloss/dt. */
int abr_feat_distill(const float* src, const float* tgt, int64_t n, float* loss_out, float* stats3, float gscale, float* d_tgt,
                     void* stream);
/* calculate_rpn_distillation_loss(cls_loss='filtered_l2', bbox_loss='l2'|'None', bbox_threshold)  distillation.py:18-84 (ablation
 * DIST.RPN), one level, NHWC head outputs: anchor a of row r has objectness obj[r*ld_obj + a] and deltas reg[r*ld_reg + 4a .. +3].
 * loss = mean_anchors max(o_s-o_t,0)^2 + mean_anchors [o_s-o_t > thr] sum_4 (d_s-d_t)^2.  d_obj_t / d_reg_t optional (same pitches
 * ld_d_obj / ld_d_reg), = gscale * dloss/d(target). */
int abr_rpn_distill(const float* obj_s, const float* reg_s, int ld_obj_s, int ld_reg_s, const float* obj_t, const float* reg_t,
                    int ld_obj_t, int ld_reg_t, int64_t rows, int A, float bbox_threshold, int use_bbox, float* loss_out,
                    float gscale, float* d_obj_t, float* d_reg_t, int ld_d_obj, int ld_d_reg, void* stream);

/* calculate_roi_distillation_losses(soften, target, dist)   distillation/distillation.py:164-240
 *   dist_id!=0 -> unbiased cross-entropy + L2 boxes ; else mean-centred L2 + L2 boxes
 * z_s [n,K_old], b_s [n,K_old,4], z_t [n,K_all], b_t [n,K_all,4]; d_zt/d_bt optional. */
/* ld_host: optional 6 row pitches (z_s, b_s, z_t, b_t, d_zt, d_bt) in floats, <=0 = dense; lets the scores / boxes
 * be column slices of the fused predictor output. */
int abr_roi_distill(const float* z_s, const float* b_s, const float* z_t, const float* b_t, int n, int K_old,
                    int K_all, const int32_t* ld_host, int dist_id, float* loss_out, float gscale, float* d_zt,
                    float* d_bt, void* stream);

/* F.binary_cross_entropy_with_logits(x[idx], y[idx]).mean()   modeling/rpn/loss.py:145-146
 * idx int64 [n_idx] into the flattened logits; grad optional, pre-zeroed, same shape as x. */
int abr_bce_logits_gather(const float* x, const float* y, const int64_t* idx, const int64_t* yidx /* NULL = idx */,
                          int n_idx, const float* denom_dev /* optional device scalar replacing n_idx as the mean's
                          denominator; idx < 0 entries are skipped (fixed-size, -1 padded index lists) */,
                          float* loss_out, float gscale, float* grad, void* stream);

/* =====================================================================================================
 * 3. Convolution as implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), NHWC / OHWI.
 *    Replaces cuDNN fwd/dgrad/wgrad + FrozenBatchNorm2d + ReLU + residual add of
 *    modeling/backbone/resnet.py:327-346,363-368, layers/batch_norm.py:19-31, modeling/rpn/rpn.py:114-121,
 *    roi_box_predictors.py:27-32 (Linear = 1x1 conv on a 1x1 map).
 * ===================================================================================================== */
#define ABR_MATH_F32 0
#define ABR_MATH_BF16 1
#define ABR_MATH_BF16X6 2
#define ABR_MATH_F16X3 3
#define ABR_MATH_F16 4

typedef struct {
    int B, H, W, Cin;        /* input  [B,H,W,Cin]  (Cin % 4 == 0) */
    int Cout, R, S;          /* weight [Cout,R,S,Cin] (OHWI)       */
    int stride, pad;
    int Ho, Wo;              /* output spatial size                 */
    /* epilogue: y = acc*scale[c] + bias[c] (+ residual) ; relu ; y *= (mask>0) */
    const float* scale;      /* [Cout] or NULL (=1)                 */
    const float* bias;       /* [Cout] or NULL (=0)                 */
    const float* residual;   /* same geometry as out, or NULL       */
    const float* mask;       /* same geometry as out, or NULL: multiply by (mask>0) (ReLU backward) */
    int relu;
    /* output placement: row (b,ho,wo) is stored at pixel (b, ho*out_sh, wo*out_sw) of [B,out_H,out_W,Cout]
       (out_sh=out_sw=1, out_H=Ho, out_W=Wo for an ordinary conv; 2 for the dgrad of a stride-2 1x1 conv) */
    int out_H, out_W, out_sh, out_sw;
    /* arithmetic of the contraction: ABR_MATH_F32 = fp32 MFMA (exact fp32, the default and the parity path);
       ABR_MATH_BF16 = both operands rounded to bf16 (RNE) inside the kernel, bf16 MFMA, fp32 accumulate, fp32 tensors in
       memory (BASELINE.json configs[4]); layers whose Cin is not a multiple of 64 (the stem) compute in fp32 either way;
       ABR_MATH_BF16X6 = fp32-ACCURATE arithmetic on the bf16 matrix cores: each fp32 operand split exactly into three bf16
       terms, the six cross products with i + j <= 2 accumulated in fp32 (same error bound as an fp32 FMA chain; opt-in);
       ABR_MATH_F16X3: see x_amax below;
       ABR_MATH_F16 = REDUCED precision on the fp16 matrix cores: each operand ROUNDED once, x ~ s fp16(x / s) with f16x3's scale s (the amax
       words below; per output row for weights), ONE v_mfma_f32_32x32x16_f16 product per multiply-add, fp32 accumulation, fp32 tensors in
       memory.  Relative representation error <= 2^-12 per operand (absolute 2^-25 s below fp16's normal range); never Winograd; layers whose
       Cin is not a multiple of 32 (the stem) compute in fp32.  Flags as under f16x3 (NONFINITE, STALE), no small-element statistics */
    int math;
    /* Winograd-domain input reuse between a convolution's forward pass and its weight gradient (both transform the SAME input
       with B^T d B).  abr_conv_forward: if wino_v is non-NULL the transformed input V (abr_conv_wino_v_floats floats) is written
       THERE instead of scratch; a conv that does not take the Winograd path, or cannot complete it, returns an error instead.
       abr_conv_wgrad: if wino_v is non-NULL and abr_conv_wino_v_floats of its descriptor is non-zero, V is read from there and
       the input transform is skipped (x is not touched).  NULL = self-contained calls. */
    float* wino_v;
    /* ABR_MATH_BF16X6 / ABR_MATH_BF16, abr_conv_forward only: the weights as FRAGMENT-PACKED bf16x3 planes made by abr_conv_pack_weights(w, Cout,
       R*S*Cin) (abr_conv_packed_bytes bytes): the weights-direct kernel then loads every weight fragment straight from these planes
       into the matrix-core registers -- no per-workgroup split, no LDS traffic for the weights.  NULL with w_version != 0: the library
       packs (w, w_version) itself on first use and keeps the planes; NULL with w_version == 0: packed into stream scratch on every call. */
    const void* w_planes;
    /* abr_conv_forward: non-zero = "the weight tensor at address w has not changed since the last call that passed this same
       (w, w_version) pair": the library then keeps data derived from it -- the Winograd-domain weights U = G g G^T (36*Cout*Cin
       floats, or their packed bf16x3 planes under ABR_MATH_BF16X6) and the packed bf16x3 planes of w -- and skips the derivation on later calls (the frozen source model: once; a trainable conv: once per optimiser
       step, shared by its forward passes).  0 = derive it again on every call. */
    int64_t w_version;
    /* ABR_MATH_F16X3 (round 5): fp32-ACCURATE contractions with THREE products per multiply-add.  Each operand is written x = s (h0 + h1) with
       h0 = fp16(x / s), h1 = fp16(x / s - h0) and s = the power of two that puts the operand's largest magnitude in [2^14, 2^15) -- per tensor
       for activations / gradients, per output channel for weights (folded into the epilogue) -- and x w = s_x s_w (h0 g0 + h0 g1 + h1 g0) runs on
       v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Representation error <= 2^-22 |x| for |x| >= 2^-18 amax (2^-40 amax below), random-signed:
       the result meets the fp32-MFMA error bound on tensors whose reductions are not made of such elements only (tests/test_gpu_f16x3_admission.py).
       The amax of an activation tensor lives in an AMAX WORD (abr_h3_amax_alloc): the producing kernel writes it (out_amax: any abr_conv_forward,
       whatever its math), the consuming kernel reads it (x_amax; gy_amax for abr_conv_wgrad).  A NULL x_amax / gy_amax makes the call reduce the
       operand itself first (one extra pass over it: correct, slower). */
    const uint64_t* x_amax;   uint32_t x_amax_epoch;
    const uint64_t* gy_amax;  uint32_t gy_amax_epoch;
    uint64_t* out_amax;       uint32_t out_amax_epoch;
} abr_conv_desc;

/* An amax word of the library's zero-initialised device ring and the epoch to use with it (see abr_conv_desc).  A word is handed out again after
 * ABR_H3_AMAX_RING allocations; by then its tensor must be gone (a reader naming an older epoch raises ABR_H3_FLAG_STALE). */
#define ABR_H3_AMAX_RING 65536
int abr_h3_amax_alloc(uint64_t** word_out, uint32_t* epoch_out);
/* n consecutive allocations at once (a host wrapper hands them out itself: one library call per n tensors instead of one per tensor):
 * allocation k of the block (0 <= k < n) is word ring_base + (first_count + k) % ABR_H3_AMAX_RING with epoch (uint32_t)(first_count + k + 1). */
int abr_h3_amax_alloc_block(int n, uint64_t** ring_base_out, uint64_t* first_count_out);
/* Range statistics of the f16x3 kernels since the last reset: out_host[0] = operand elements seen more than 18 binades below their tensor's amax
 * (non-zero), out_host[1] = operand elements inspected (every element of an activation / gradient operand once per GEMM).  Synchronises `stream`. */
int abr_h3_range_stats(uint64_t* out_host, int reset, void* stream);
/* the same two numbers written to DEVICE memory on `stream` without synchronising (a training loop copies them out asynchronously, after a SUM
 * over the ranks under data parallelism: engine/trainer.py::_x6_guard) */
int abr_h3_range_stats_to_device(uint64_t* out_device, int reset, void* stream);
/* *word = (epoch << 32) | bits(max |x[i]|) for n floats on `stream` (what a producer kernel's epilogue writes for free) */
int abr_h3_amax(const float* x, int64_t n, uint64_t* word, uint32_t epoch, void* stream);
/* *out_word = (out_epoch << 32) | max over l < L of the amax bits in words_host[l] (each read under epochs_host[l]), one one-wave launch on
 * `stream` (csrc/box_head_fpn.hip): an upper bound of max |x| for a tensor whose every value is bounded by one of L tagged tensors -- the
 * multi-level Pooler's output, each row an average of bilinear samples of one of the L maps.  words_host / epochs_host are HOST arrays of L
 * entries copied into the kernel's arguments; 1 <= L <= ABR_MAX_PYRAMID_LEVELS; out_word a fresh word (abr_h3_amax_alloc*), none of the L.
 * The L words must have been written on `stream` or ahead of it.  If one of them no longer carries its epoch the output word is NOT written:
 * its reader then raises ABR_H3_FLAG_STALE, as a reader of that level's own word would.  Written with the protocol's 64-bit atomic max. */
int abr_h3_amax_max(const uint64_t* const* words_host, const uint32_t* epochs_host, int L, uint64_t* out_word, uint32_t out_epoch, void* stream);

int abr_conv_forward(const abr_conv_desc* d_host, const float* x, const float* w, float* out, void* stream);
/* The tail of a 64-wide bottleneck WITHOUT a backward pass (maskrcnn_benchmark/modeling/backbone/resnet.py:327-346 for the frozen layer1:
 * conv2 3x3 -> bn2 -> relu -> conv3 1x1 -> bn3 -> += identity -> relu) as ONE launch: d2 = the 3x3 conv (64 -> 64, stride 1, pad 1, scale / bias /
 * relu as in abr_conv_forward), d3 = the 1x1 conv (64 -> 256, scale / bias / residual / relu), both ABR_MATH_BF16X6 with w_version != 0 (or
 * caller-packed w_planes).  out [B,H,W,256] is bit-identical to abr_conv_forward(d2) followed by abr_conv_forward(d3); the intermediate tensor
 * never leaves the compute unit. */
int abr_conv_tail64_forward(const abr_conv_desc* d2_host, const abr_conv_desc* d3_host, const float* x, const float* w2, const float* w3, float* out,
                            void* stream);
/* Derive, on `stream`, whatever abr_conv_forward would derive from the weight tensor (w, w_version != 0) of a conv with this geometry and
 * arithmetic -- the Winograd-domain weights of a wide stride-1 3x3 conv, the packed bf16x3 planes of any bf16x6 conv -- so that the next abr_conv_forward with the same
 * (w, w_version) finds it ready (a consumer on another stream is ordered behind it by the library).  Lets a
 * caller move the per-step weight preparation of its trainable convs off the critical stream (solver/build.py). */
int abr_conv_prepare_weights(const float* w, int Cout, int R, int S, int Cin, int stride, int pad, int math, int64_t w_version, void* stream);
/* The same for a whole model in a handful of launches.  Item i: what abr_conv_prepare_weights derives from w; and, when wt != NULL, first the
 * dgrad copy wt = abr_conv_dgrad_weights(w, scale) and then what abr_conv_prepare_weights(wt, Cin -> Cout swapped, stride 1, pad R-1-pad) derives
 * from THAT.  All transposes go out as one launch, all Winograd weight transforms as one, all bf16x3 packings as one (a model's ~190 per-tensor
 * launches after every optimiser step were a host-paced train of tiny kernels and ~3 ms of host time).  Results and cache entries are
 * the ones the per-tensor calls produce.  Items whose shape the batched kernels do not take (Cin % 4 != 0 Winograd weights) go the per-tensor way. */
typedef struct abr_prep_item {
    const float* w;       /* [Cout][R][S][Cin] */
    const float* scale;   /* FrozenBN scale folded into the dgrad copy, or NULL */
    float* wt;            /* [Cin][R][S][Cout] dgrad copy (flipped taps), or NULL: forward derivation only */
    int32_t Cout, R, S, Cin, stride, pad, math;
    int64_t w_version;
} abr_prep_item;
int abr_conv_prepare_batch(const abr_prep_item* items_host, int n, void* stream);

/* A table of conv calls in ONE library call (round 5: the host side of a bottleneck's forward or backward pass is four to ten of the calls above,
 * ~12 us of interpreter and binding time each; a host wrapper keeps the table of a (block, input shape) with everything that does not change from
 * step to step filled in and writes only this step's pointers).  Ops run in table order, each on ITS stream:
 *   ABR_OP_FORWARD      abr_conv_forward(&desc, a = x, b = w, out, stream)
 *   ABR_OP_WGRAD        abr_conv_wgrad(&desc, a = x, b = gy, out = dw, stream)
 *   ABR_OP_STREAM_WAIT  abr_stream_wait_stream(stream, other)            -- `stream` waits for what `other` has queued so far
 * Stops at the first failing op and returns its status (abr_last_error names it).  The reference's counterpart: one cuDNN call per conv from
 * ATen, driven by the Python of modeling/backbone/resnet.py:327-346. */
#define ABR_OP_FORWARD 0
#define ABR_OP_WGRAD 1
#define ABR_OP_STREAM_WAIT 2
typedef struct abr_conv_op {
    int32_t kind;
    int32_t reserved;
    abr_conv_desc desc;
    const float* a;
    const float* b;
    float* out;
    void* stream;
    void* other;
} abr_conv_op;
int abr_conv_run(const abr_conv_op* ops, int n);
/* The library keeps this derived data per (weight address, kind, w_version) -- 36/9 of each wide 3x3 weight, 1.5x of every other bf16x6 weight.  The cache is bounded
 * (least-recently-used entries go when it exceeds ABR_WINO_CACHE_MB, default 4096); abr_conv_cache_clear drops every entry after waiting
 * for the streams that use them (call it when a model's parameter storage is released or rebuilt), abr_conv_cache_bytes reports its size. */
int abr_conv_cache_clear(void);
/* the same for the entries derived from tensors that live inside [base, base + bytes) only (a model's flat parameter storage that is being
 * released): entries of other models -- and conv calls in flight on other host threads that hold them -- are not touched.  Both calls skip
 * entries whose fill is in progress on another thread. */
int abr_conv_cache_drop_range(const void* base, int64_t bytes);
int64_t abr_conv_cache_bytes(void);
/* bytes of the device memory the library owns besides that cache: its per-stream scratch (grow-only, one buffer per user and stream) and its
 * process-wide words (range flags, f16x3 statistics, the amax ring).  DESIGN.md, "Library-owned scratch". */
int64_t abr_scratch_bytes(void);
/* floats of the Winograd-domain input V = 36 * B*ceil(H/4)*ceil(W/4) * Cin if BOTH abr_conv_forward and abr_conv_wgrad take the
 * Winograd F(4x4,3x3) path for this descriptor (wide stride-1 pad-1 3x3, no residual / scatter; fp32 math, or bf16x6 / f16x3 with
 * Cout % 32 == 0), else 0 */
int64_t abr_conv_wino_v_floats(const abr_conv_desc* d_host);
/* What the library decided for this descriptor (host only, no device call): out = { the arithmetic the forward pass runs in (ABR_MATH_*: fp32 for
 * a split arithmetic with Cin % 32 != 0 and for bf16 with Cin % 64 != 0), 1 if abr_conv_forward takes Winograd F(4x4,3x3), 1 if abr_conv_wgrad
 * does, the arithmetic of the weight gradient }.  The forward entries follow d_host's residual pointer and scatter geometry. */
int abr_conv_route_info(const abr_conv_desc* d_host, int32_t out[4]);
/* Fragment-packed bf16x3 planes of an fp32 matrix w [rows][K] (K % 16 == 0; a conv weight: rows = Cout, K = R*S*Cin) for
 * abr_conv_desc::w_planes.  Exact three-way split x = p0 + p1 + p2 (p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), RNE), stored in
 * the order the bf16 MFMA consumes it: chunk (nb, ks, pl) = 64 lanes x 16 B at byte (((nb * K/16 + ks) * 3 + pl) * 64 + lane) * 16, lane l
 * holding row nb*32 + (l & 31), k = ks*16 + (l >> 5)*8 .. +8 of plane pl; rows are zero-padded to a multiple of 32.  The elements are
 * range-checked for the bf16x6 arithmetic as they are packed (abr_x6_range_flags). */
int64_t abr_conv_packed_bytes(int64_t rows, int64_t K);
int abr_conv_pack_weights(const float* w, int64_t rows, int K, void* planes, void* stream);

/* dW[Cout,R,S,Cin] (+)= sum_m gy[m,Cout]^T * im2col(x)[m,RSCin], columns scaled by d->scale (FrozenBN).
 * Accumulates with fp32 atomics into dw (caller zeroes it once per step). */
int abr_conv_wgrad(const abr_conv_desc* d_host, const float* x, const float* gy, float* dw, void* stream);

/* w [Cout,R,S,Cin] -> wt [Cin,R,S,Cout] spatially flipped and scaled by scale[Cout]: the weight tensor
 * that turns dgrad into abr_conv_forward(gy, wt). */
int abr_conv_dgrad_weights(const float* w, const float* scale, int Cout, int R, int S, int Cin, float* wt,
                           void* stream);
/* db[c] += sum_m gy[m,c] (bias gradient of nn.Conv2d / nn.Linear) */
int abr_bias_grad(const float* gy, int64_t M, int C, float* db, void* stream);

/* =====================================================================================================
 * 4. Pointwise / pooling / layout
 * ===================================================================================================== */
int abr_nchw_to_nhwc_pad(const float* x, int B, int C, int H, int W, int Cpad, float* out, void* stream);
int abr_nhwc_to_nchw(const float* x, int B, int C, int H, int W, float* out, void* stream);
int abr_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float* out, void* stream);
int abr_maxpool3x3s2(const float* x, int B, int H, int W, int C, float* out, void* stream); /* resnet.py:367 */
/* its backward fused with the ReLU that produced x (the stem's y [B,H,W,C]): g_y = (y <= 0 ? 0 : sum of g_pool [B,Ho,Wo,C] over the windows
 * whose selected element -- maxpool's rule: first maximum in (dy, dx) order, a NaN wins -- is this pixel).  Gather form, deterministic; writes all of g_y */
int abr_maxpool3x3s2_backward(const float* y, const float* g_pool, int B, int H, int W, int C, float* g_y, void* stream);
/* Deformable 3x3 conv (stride 1, pad 1; DCNv1, and DCNv2 = modulated with one deformable group) as columns for the 1x1 conv route.
 * x [B,H,W,C], om [B,H,W,Com] (offset / mask field: dh of tap k = 3i+j and group g at 2k+18g, dw at 2k+1+18g; v2: mask logit of tap k at 18+k)
 * -> cols [B,H,W,9C] (tap outermost): cols = m * bilinear(x, ho-1+i+dh, wo-1+j+dw), 0 outside the open box -1 < h < H, -1 < w < W.
 * C / dg % 4 == 0. */
int abr_deform_im2col(const float* x, const float* om, int B, int H, int W, int C, int Com, int dg, int modulated, float* cols, void* stream);
/* its backward from dcol [B,H,W,9C]: dx [B,H,W,C] += the bilinear scatter of m * dcol (fp32 atomics: the caller zeroes dx; the order of the adds
 * varies from run to run), d_om [B,H,W,Com] = d/d(dh, dw) and, under v2, d/d(mask logit), summed over each group's channels in a fixed order
 * (deterministic); channels past the field's 18 dg (v2: 27) are written as 0.  d_om_amax (optional): max |d_om| into that amax word.
 * C a power of two in [4, 1024]. */
int abr_deform_col2im_coord(const float* dcol, const float* x, const float* om, int B, int H, int W, int C, int Com, int dg, int modulated,
                            float* dx, float* d_om, uint64_t* d_om_amax, uint32_t d_om_amax_epoch, void* stream);
/* The general deformable conv (_C.deform_conv_* / _C.modulated_deform_conv_*: csrc/deform_conv.h, deform_conv_kernel_cuda.cu:198-460 and
 * :578-780, restated) as columns: any kernel with kh * kw <= 49, stride, padding, dilation, `groups` conv groups and `dg` deformable groups.
 * x [B,H,W,C], offset [B,Ho,Wo,dg*2*K] (K = kh*kw; for deformable group g = C/dg consecutive channels and tap k = i*kw + j: dh at
 * g*2K + 2k, dw at g*2K + 2k + 1), mask [B,Ho,Wo,dg*K] or NULL (the factor of group g and tap k at g*K + k, used as given: no sigmoid)
 * -> cols [groups][B*Ho*Wo][K * C/groups], group-major, tap outermost and channel innermost inside a group: each group is the operand of
 * a 1x1 conv with the OHWI weight read as [Cout/groups][K * C/groups].
 * Sample point in fp32: h = ho*stride_h - pad_h + i*dil_h + dh, w = wo*stride_w - pad_w + j*dil_w + dw; the value is 0 unless -1 < h < H and
 * -1 < w < W (non-finite and huge coordinates are outside), else the bilinear interpolation of the corners floor, floor + 1, a corner outside
 * the image contributing 0; cols = mask * value.
 * Refused before any launch (negative status, abr_last_error names the argument): kh*kw > 49; non-positive sizes; C % groups or C % dg
 * non-zero; C/groups or C/dg not a multiple of 4; B*Ho*Wo*K*C/4 >= 2^31; Ho or Wo other than (H + 2 pad - (dil (k - 1) + 1)) / stride + 1. */
int abr_deform_im2col_general(const float* x, const float* offset, const float* mask, int B, int H, int W, int C, int Ho, int Wo, int kh, int kw,
                              int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int groups, int dg, float* cols,
                              void* stream);
/* its backward from dcol (cols' shape).  dx [B,H,W,C] is ADDED INTO with fp32 atomics (the caller zeroes it, or passes a gradient to
 * accumulate into; the order of the adds varies from run to run; one wave instruction adds the consecutive channels of one corner pixel,
 * 256 contiguous bytes once C/dg >= 64).  d_offset [B,Ho,Wo,dg*2*K] (the derivative with the floors held fixed, zero outside the open box)
 * and d_mask [B,Ho,Wo,dg*K] (sum over the group's channels of dcol * value; NULL exactly when mask is) are WRITTEN, every element by its one
 * owner, summed over the group's channels in a fixed order: no atomics, bit-reproducible.  The same refusals. */
int abr_deform_col2im_coord_general(const float* dcol, const float* x, const float* offset, const float* mask, int B, int H, int W, int C, int Ho,
                                    int Wo, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int groups,
                                    int dg, float* dx, float* d_offset, float* d_mask, void* stream);
/* AdaptiveAvgPool2d(1)  roi_box_predictors.py:28 : x [N,HW,C] -> out [N,C] ; backward spreads g/HW */
int abr_avgpool_forward(const float* x, int N, int HW, int C, float* out, void* stream);
int abr_avgpool_backward(const float* g, int N, int HW, int C, float* gx, void* stream);
/* the same fused with the backward of the ReLU that produced the pooled tensor y [N, HW, C]: gx = y > 0 ? g / HW : 0 */
int abr_avgpool_relu_backward(const float* g, const float* y, int N, int HW, int C, float* gx, void* stream);
/* ... which also writes max |gx| into an amax word (abr_h3_amax_alloc) for the f16x3 convs that consume gx; amax == NULL: as above */
int abr_avgpool_relu_backward_amax(const float* g, const float* y, int N, int HW, int C, float* gx, uint64_t* amax, uint32_t amax_epoch, void* stream);
/* out[row] = mean_c x[row, c] for x [rows, C] -- per-(RoI, bin) channel mean of NHWC pooled features
 * (tools/prototype_box_selection.py:84 `torch.mean(roi_align_features, dim=1)`) */
int abr_channel_mean(const float* x, int64_t rows, int C, float* out, void* stream);
/* out = g * (y > 0)  (ReLU backward); out == g is allowed (in place) */
int abr_relu_backward(const float* g, const float* y, int64_t n, float* out, void* stream);
int abr_add_inplace(float* a, const float* b, int64_t n, void* stream);
/* The training loop's loss arithmetic (tools/train_incremental.py:91,101-128: sum of the detector losses, alpha * ID + beta * ARD, their sum)
 * in one launch: terms_host [n <= 8] HOST array of DEVICE pointers to the scalar losses, weights_host / groups_host [n] host arrays
 * (group 0 = detector losses, 1 = distillation); *total = out[0] = sum w_i l_i, out[1] / out[2] = the two groups' sums.  The backward hands
 * every term its gradient w_i * *g (g: device scalar) in one launch. */
int abr_loss_sum(const float* const* terms_host, const float* weights_host, const int32_t* groups_host, int n, float* total, float* out,
                 void* stream);
int abr_loss_sum_backward(const float* weights_host, int n, const float* g, float* grads, void* stream);
/* x *= s * (s_dev ? *s_dev : 1): applies an upstream (device-resident) loss gradient without a host sync */
int abr_scale_inplace(float* x, int64_t n, float s, const float* s_dev, void* stream);

/* =====================================================================================================
 * 5. RPN / RoI-head glue (integer + fp32 index work; maskrcnn_benchmark/modeling/rpn/, matcher.py, box_coder.py)
 * ===================================================================================================== */
/* AnchorGenerator grid  anchor_generator.py:84-110 : out [H*W*A,4], vis [H*W*A] uint8 */
int abr_grid_anchors(const float* cell, int A, int H, int W, int stride, int img_h, int img_w, int straddle,
                     float* out, uint8_t* vis, void* stream);
/* sigmoid + top-k (sorted, descending; ties by ascending index) of the RPN objectness, per image, in one launch
 * (rpn/inference.py:87-96).  Anchor j of image i is logits[i*img_stride + (j/A)*ld + j%A] (A=15, ld=76 on the fused NHWC head
 * output; A=1, ld=1 for a plain [N,n] matrix).  scores [N,k] fp32, idx [N,k] int64.  k <= 15360. */
int abr_topk_sigmoid(const float* logits, int64_t img_stride, int N, int n, int A, int ld, int k, float* scores,
                     int64_t* idx, void* stream);
/* Test-time PostProcessor, stage 1 (roi_heads/box_head/inference.py:55-70, box_coder.py:52-95, bounding_box.py:214-225):
 * prob = softmax(logits[:, :C]); boxes[r,j] = clip_to_image(decode(deltas[r, delta_col0 + 4j .. +3], rois[r,1:5])).
 * rois [K,5] = (image index, x1,y1,x2,y2); img_hw [N,2] int32 (h,w).  agnostic_col >= 0 (CLS_AGNOSTIC_BBOX_REG): every class
 * reads the 4 columns at delta_col0 + agnostic_col instead.  prob [K,C], boxes [K,C,4]. */
int abr_det_softmax_decode(const float* logits, int ld_logits, const float* deltas, int ld_deltas, int delta_col0,
                           int agnostic_col, const float* rois, int K, int C, const int32_t* img_hw, float wx, float wy,
                           float ww, float wh, float* prob, float* boxes, void* stream);
/* Test-time PostProcessor, stage 2 = filter_results (inference.py:106-151) for the whole batch: per image and class
 * score > score_thresh, sort, NMS (`>=` as the CPU _C.nms), classes 1..C-1 concatenated, and when more than
 * detections_per_img (> 0) remain only those with score >= the detections_per_img-th largest (ties kept, order kept).
 * row_offsets [N+1] int32 (device): rows of image i in prob/boxes; r_max >= every image's row count (<= 16384).
 * out_* [N,cap,...] (cap = (C-1)*r_max holds every case), out_labels int64, out_count [N] int32.
 * bg_* [N,r_max,...] / bg_count [N]: class 0's NMS survivors (the reference's `results_background`); NULL to skip. */
int64_t abr_det_select_workspace_bytes(int N, int C, int r_max);
int abr_det_select(const float* prob, const float* boxes, const int32_t* row_offsets, int N, int C, int r_max,
                   float score_thresh, float nms_thresh, int detections_per_img, int cap, float* out_boxes,
                   float* out_scores, int64_t* out_labels, int32_t* out_count, float* bg_boxes, float* bg_scores,
                   int32_t* bg_count, void* workspace, int64_t workspace_bytes, void* stream);
/* BoxCoder.decode + clip_to_image on gathered rows  (rpn/inference.py:96-112, box_coder.py:52-95, bounding_box.py:214-225)
 * For image i and rank j<k: a = idx[i,j]; out[i,j,:] = clip(decode(reg[i,a,:], anchors[a,:])).
 * reg [N,n_anchor/A,reg_stride]: anchor a = loc*A + a' reads columns reg_col0 + 4a' .. +3 of row loc
 * (A=1: one row per anchor; A=15, reg_stride=76, reg_col0=15: the fused NHWC RPN head output). */
int abr_rpn_decode_clip(const float* reg, int reg_stride, int reg_col0, int A, const float* anchors,
                        const int64_t* idx, int N, int n_anchor, int k, const int32_t* img_hw, float wx,
                        float wy, float ww, float wh, float* out, void* stream);
/* RPN proposal selection over a feature pyramid (rpn/inference.py:76-118 per level, :120-176 across the levels), S = N * L (image, level)
 * segments, segment s = i * L + l, through every stage together and nothing read back (csrc/rpn_pyramid.hip):
 *   abr_rpn_pyramid_topk -> abr_rpn_pyramid_decode -> abr_nms_sorted_batched(props, counts, S, k_max, thr, 0, post, ...) -> abr_rpn_pyramid_select.
 * y_host[l] = device pointer of level l's fused head output [N, nloc[l], ld[l]] (row = location; columns 0 .. A[l]-1 the logits of anchors
 * loc * A + a, columns A[l] + 4a .. +3 their deltas, further columns never read); y_host, nloc_host, A_host, ld_host, anchors_host are HOST arrays
 * of L entries copied into the kernels' arguments.  1 <= L <= ABR_MAX_PYRAMID_LEVELS; k_l = min(pre_nms_top_n, nloc[l] * A[l]) and k_max = max k_l,
 * else an error; the ranking (not the decode) also needs k_l <= abr_rpn_pyramid_max_k() (2048: the in-LDS sort, 32 KB of LDS per workgroup) --
 * beyond it a caller ranks level by level with abr_topk_sigmoid into the same tables; the keys of all levels, N * L * k_max * 4 and
 * N * L * post must fit int32.  N == 0 launches nothing.  The number of launches does not depend on N or L. */
int abr_rpn_pyramid_max_k(void);
/* scores [N,L,k_max] fp32, idx [N,L,k_max] int64 level-local anchor ids: per segment the k_l largest sigmoid(logit), descending, equal scores by
 * ascending index -- bit for bit what abr_topk_sigmoid returns for that level alone; entries k_l .. k_max-1 are 0. */
int abr_rpn_pyramid_topk(const float* const* y_host, const int* nloc_host, const int* A_host, const int* ld_host, int L, int N, int pre_nms_top_n,
                         int k_max, float* scores, int64_t* idx, void* stream);
/* BoxCoder.decode + clip_to_image of the ranked anchors (ld[l] >= 5 A[l]; anchors_host[l] = device [nloc*A,4]) through the one decode and clip
 * that abr_rpn_decode_clip and abr_det_softmax_decode call too (csrc/box_math.h), so the three agree bit for bit on the same inputs,
 * then remove_small_boxes (boxlist_ops.py:34-48: keep iff x2-x1+1 >= min_size and y2-y1+1 >= min_size; min_size <= 0 keeps every row) and a stable
 * compaction: props [S,k_max,4] / scores_out [S,k_max] hold each segment's survivors in rank order without holes (rows past the count: 0),
 * counts [S] int32 (device; may be 0).  img_hw [N,2] int32 (h, w). */
int abr_rpn_pyramid_decode(const float* const* y_host, const int* nloc_host, const int* A_host, const int* ld_host, const float* const* anchors_host,
                           int L, int N, int pre_nms_top_n, int k_max, const int64_t* idx, const float* scores_in, const int32_t* img_hw, float wx,
                           float wy, float ww, float wh, float min_size, float* props, float* scores_out, int32_t* counts, void* stream);
/* select_over_all_levels (inference.py:149-176).  keep [S,post] / n_keep [S] = abr_nms_sorted_batched's output over props / scores [S,k_max,..].
 * Candidates of image i: its levels' NMS survivors in level order, each level in keep order; candidate position p = level * post + rank.
 *   mode 0 (test, or training per image): the min(fpn_post_n, #candidates) highest scores per image, emitted by descending score;
 *   mode 1 (training per batch): the min(fpn_post_n, #candidates of all images) highest scores of the batch; every image emits its chosen
 *          candidates in candidate order (the reference indexes with a mask).
 * torch.topk leaves a tie group's members undefined; here equal scores go by ascending candidate position, image-major in mode 1.  The cut is an
 * exact radix selection on (order-preserving score key, position), so no result depends on the order in which atomics were won.
 * cap = min(fpn_post_n, L * post) (<= 4096 in mode 0: the in-LDS sort): rois [N,cap,4], out_scores [N,cap], src [N,cap] int32 = p (-1 past the
 * count), n_out [N] int32.  Scores may be any non-NaN fp32. */
int abr_rpn_pyramid_select(const float* props, const float* scores, const int32_t* keep, const int32_t* n_keep, int N, int L, int k_max, int post,
                           int fpn_post_n, int mode, float* rois, float* out_scores, int32_t* src, int32_t* n_out, void* stream);
/* RetinaNet's test-time post-processor over a feature pyramid (rpn/retinanet/inference.py:73-123 per level, :131-174 across the levels), S = N * L
 * (image, level) segments, through every stage together and nothing read back (csrc/retinanet.hip): 1 memset + 4 launches whatever N, L and C are.
 * cls_host[l] = device pointer of level l's class logits [N, nloc[l], ldc[l]] (row = location; column a * C + c the logit of anchor loc * A + a and
 * class c + 1, columns >= A * C never read), reg_host[l] = its deltas [N, nloc[l], ldr[l]] (columns 4a .. 4a+3 anchor a's, further columns never
 * read), anchors_host[l] = device [nloc[l] * A, 4]; the six tables are HOST arrays of L entries copied into the kernels' arguments.  A anchors per
 * location and C = NUM_CLASSES - 1 foreground classes are shared by the levels: there is one head.  img_hw [N,2] int32 (h, w).
 *   a. per segment: score = sigmoid(x) in fp32 by abr_topk_sigmoid's formula; a logit is a candidate iff score > score_thresh; the
 *      min(#candidates, pre_nms_top_n) highest are kept by descending score.  torch.topk(sorted=False) leaves ties undefined: here equal scores go
 *      by ascending flat index loc * A * C + a * C + c.
 *   b. anchor = flat / C, label = flat % C + 1; BoxCoder(wx, wy, ww, wh).decode and clip_to_image through the one decode and clip of csrc/box_math.h
 *      (bit for bit abr_rpn_pyramid_decode's), remove_small_boxes(min_size) (min_size <= 0 keeps every row), stable compaction in rank order.
 *   c. per image: for each class 1 .. C in turn its candidates of all levels by descending score -- equal scores by ascending candidate position
 *      level * pre_nms_top_n + rank -- through greedy NMS at nms_thresh with abr_nms_sorted_batched's `>=` rule (strict_gt = 0); the survivors
 *      concatenated class by class; when more than detections_per_img (> 0; <= 0: no limit) remain only those with score >= the
 *      detections_per_img-th largest (ties at the cut all kept, order unchanged).
 * Every cut is an exact radix selection on unique words, every list is compacted in order: no result depends on which workgroup won an atomic.
 * out_boxes [N,cap,4], out_scores [N,cap], out_labels [N,cap] int64, n_out [N] int32 (device), rows past the count 0; cap = L * pre_nms_top_n holds
 * every case, ties included.  Limits, checked before any launch (else ABR_E_INVALID): 1 <= L <= ABR_MAX_PYRAMID_LEVELS, pre_nms_top_n <=
 * abr_rpn_pyramid_max_k() (2048), L * pre_nms_top_n <= abr_retina_max_candidates() (8192: the per-image sort in LDS; the defaults need 5 x 1000),
 * C <= 524286, every level's nloc * A * C and N * nloc * ld in int32, N * L <= 65535.  N == 0 launches nothing. */
int abr_retina_max_candidates(void);
int abr_retina_detect(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host,
                      const float* const* anchors_host, const int* nloc_host, int L, int N, int A, int C, const int32_t* img_hw, float score_thresh,
                      int pre_nms_top_n, float nms_thresh, int detections_per_img, float wx, float wy, float ww, float wh, float min_size, int cap,
                      float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* n_out, void* stream);
/* RetinaNet's training targets for the whole batch (rpn/retinanet/loss.py with rpn/loss.py:66-102; csrc/retinanet_loss.hip): Matcher(hi, lo,
 * allow_low_quality_matches = True), copied_fields = ['labels'], discard_cases = ['between_thresholds'] only -- there is NO visibility discard.
 * anchors [n,4]: the levels' anchors concatenated, shared by the images (n = A * sum nloc[l]); gt_ptrs / gt_label_ptrs: device arrays of N device
 * pointers ([G_i,4] fp32, [G_i] int64); n_gt [N] int32 (device), g_max >= max G_i.
 *   labels [N,n] int32: the class of the matched ground truth (first maximum wins), 0 background (best IoU < lo), -1 ignored (lo <= best < hi and
 *     no low-quality match);  reg_targets [N,n,4] = BoxCoder(wx, wy, ww, wh).encode(gt[max(m, 0)], anchor);  n_pos [1] int32 = the number of
 *     labels > 0 over the batch (integer counting: deterministic).
 * Through the one matcher, label rule and box coder of csrc/box_math.h.  An image with G_i == 0 (the reference crashes there): every anchor gets
 * label 0 and zero targets, and neither of its ground-truth tables is read.  2 memsets + 2 launches, no host synchronisation; N == 0 launches
 * nothing.  N * n in int32, N <= 65535, anchors and reg_targets 16-byte aligned, else ABR_E_INVALID before any launch. */
int abr_retina_targets(const float* anchors, int n, int N, const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt,
                       int g_max, float hi, float lo, float wx, float wy, float ww, float wh, int32_t* labels, float* reg_targets, int32_t* n_pos,
                       void* stream);
/* RetinaNet's loss over a feature pyramid (rpn/retinanet/loss.py:44-84; csrc/retinanet_loss.hip), read where the head left its outputs.  The level
 * tables are abr_retina_detect's: cls_host[l] = [N, nloc[l], ldc[l]] (column a * C + c the logit of anchor loc * A + a and class c + 1, columns
 * >= A * C never read), reg_host[l] = [N, nloc[l], ldr[l]] (columns 4a .. 4a+3); HOST arrays of L entries copied into the kernel's arguments.
 * labels / reg_targets / n_pos as abr_retina_targets leaves them, anchor (l, loc, a) of image i at i * n + A * sum_{m<l} nloc[m] + loc * A + a.
 *   losses[0] = sum of focal(x, label; gamma, alpha) over every anchor with label >= 0 and every class / float(n_pos + N)
 *   losses[1] = sum of smooth_l1(beta) over the four deltas of the anchors with label > 0 / max(1, n_pos * regress_norm)
 * both divided on the device.  The focal element is abr_sigmoid_focal_forward's (csrc/focal.h).  One launch; the sums go through per-workgroup
 * partials added in a fixed order (no float atomics): the same inputs give the same bits, whatever else runs.
 * Limits, checked before any launch (else ABR_E_INVALID): 1 <= L <= ABR_MAX_PYRAMID_LEVELS, C >= 1, 1 <= A <= 4096, ldc >= A * C, ldr >= 4A, both
 * % 4 == 0, every N * nloc * ld and N * n in int32, beta > 0, non-null tables, 16-byte aligned outputs of the head.  N == 0 launches nothing. */
int abr_retina_loss(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host, const int* nloc_host,
                    int L, int N, int A, int C, const int32_t* labels, const float* reg_targets, const int32_t* n_pos, float gamma, float alpha,
                    float beta, float regress_norm, float* losses, void* stream);
/* Its gradient, recomputed from the logits (the forward parks nothing).  g_cls / g_reg: the upstream gradients of the two losses (device scalars,
 * no sync).  d_cls / d_reg: ONE allocation each, level l the [N, nloc[l], ld[l]] block at float offset N * sum_{m<l} nloc[m] * ld[m] (16-byte
 * aligned as ld % 4 == 0).  One launch of plain 16-byte stores that writes EVERY element: no memset, no scatter, no atomics.
 *   d_cls = focal'(x) * s, s = g_cls / float(n_pos + N) formed once in fp32 (the element of abr_sigmoid_focal_backward with d_losses = s: the
 *     same bits); exactly 0 for ignored anchors and in the pad columns.
 *   d_reg = smooth_l1'(beta) * (g_reg / max(1, n_pos * regress_norm)) at the deltas of the anchors with label > 0, exactly 0 elsewhere.
 * Same argument checks. */
int abr_retina_loss_backward(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host,
                             const int* nloc_host, int L, int N, int A, int C, const int32_t* labels, const float* reg_targets,
                             const int32_t* n_pos, float gamma, float alpha, float beta, float regress_norm, const float* g_cls,
                             const float* g_reg, float* d_cls, float* d_reg, void* stream);
/* The RPN loss over a feature pyramid (rpn/loss.py:104-148 with rpn/utils.py:10-45; csrc/rpn_pyramid_loss.hip).  y_host[l] = device pointer of
 * level l's fused head output [N, nloc[l], Cf] (columns 0 .. A-1 the logits of anchors loc * A + a, A + 4a .. +3 their deltas; A, Cf and N are
 * shared by the levels: there is one head); y_host / nloc_host are HOST arrays of L entries copied into the kernel's arguments.  An image's anchors
 * are the levels' concatenated, n = A * sum nloc[l]: flat index g -> image g / n, j = g % n, the level l with off_l <= j < off_{l+1}
 * (off_l = A * sum_{m<l} nloc[m]), location (j - off_l) / A, anchor (j - off_l) % A.  labels [N,n] fp32, reg_targets [N,n,4]; pos [N,max_pos],
 * neg [N,batch] int64 and counts [N,2] int32 exactly as abr_sample_pos_neg leaves them with index_offset_per_image = n (-1 pads; an index outside
 * 0 .. N*n-1 is skipped like padding).  losses[0] = sum of BCE-with-logits over all listed anchors / D, losses[1] = sum of smooth_l1(beta = 1/9)
 * over the listed positives' four deltas / D, D = max(sum counts, 1), divided on the device.  One launch of one workgroup with a fixed order of
 * additions: the values do not depend on the stream or on what else runs.
 * rec_dst / rec_val (both or neither; NULL: no gradient wanted) receive the gradient as compact records, slot s = position in (pos, then neg),
 * S = N * (max_pos + batch), P = N * max_pos:  rec_dst[s] = float offset of the slot's logit in the gradient storage (-1: padding), rec_val[s] =
 * (sigmoid(x) - y) / D;  rec_dst[S + p] = offset of positive p's first delta, rec_val[S + 4p .. +3] = the smooth-L1 derivatives / D.
 * rec_dst: S + P int64, rec_val: S + 4P floats.
 * 1 <= L <= ABR_MAX_PYRAMID_LEVELS, Cf >= 5A, Cf % 4 == 0, non-null tables, else ABR_E_INVALID before any launch. */
int abr_rpn_pyramid_loss(const float* const* y_host, const int* nloc_host, int L, int N, int A, int Cf, const float* labels,
                         const float* reg_targets, const int64_t* pos, int max_pos, const int64_t* neg, int batch, const int32_t* counts,
                         float* losses, int64_t* rec_dst, float* rec_val, void* stream);
/* The dense gradient of all levels from abr_rpn_pyramid_loss's records.  grad = ONE allocation of Cf * N * sum nloc[l] floats, level l the
 * [N, nloc[l], Cf] block at float offset Cf * N * sum_{m<l} nloc[m] (16-byte aligned as Cf % 4 == 0).  One hipMemsetAsync over the allocation and
 * one scatter launch: record value * upstream gradient of its loss (g_obj, g_box: device scalars, no sync).  The sampled anchors are distinct and
 * the logit and delta columns disjoint: plain stores, everything else (pad columns included) is exactly 0.  Same argument checks. */
int abr_rpn_pyramid_loss_backward(const int* nloc_host, int L, int N, int A, int Cf, const int64_t* rec_dst, const float* rec_val, int max_pos,
                                  int batch, const float* g_obj, const float* g_box, float* grad, void* stream);
/* BoxCoder.encode row-wise (box_coder.py:22-50): out[i] = encode(gt[i], ex[i]); img_hw==NULL above = decode without clip */
int abr_box_encode(const float* gt, const float* ex, int n, float wx, float wy, float ww, float wh, float* out,
                   void* stream);
/* boxlist_iou + Matcher (+ RPN labels / box-head labels) + BoxCoder.encode in one pass per box.
 *   boxes [n,4], gt [G,4], gt_labels [G] int64 (or NULL for RPN), vis [n] uint8 (or NULL)
 *   matched [n] int64 (-1 / -2 / gt index), labels_out [n] (fp32 for RPN: 1/0/-1; int64 for head: class/0/-1),
 *   reg_targets [n,4].   matcher.py:42-112, rpn/loss.py:66-102, box_head/loss.py:56-84 */
int abr_match_encode(const float* boxes, int n, const float* gt, const int64_t* gt_labels, int G,
                     const uint8_t* vis, float hi, float lo, int allow_low_quality, float wx, float wy,
                     float ww, float wh, int64_t* matched, float* labels_f32, int64_t* labels_i64,
                     float* reg_targets, void* workspace, int64_t workspace_bytes, void* stream);
int64_t abr_match_workspace_bytes(int n, int G);

/* BalancedPositiveNegativeSampler (balanced_positive_negative_sampler.py:19-77) for N images in one launch, no host sync:
 * labels [N, n] (row pitch `stride`; fp32 for the RPN, int64 for the box head): >=1 positive, ==0 negative, else ignored.
 * Draws min(#pos, max_pos) positives and min(#neg, batch_size - that) negatives uniformly at random (counter-based keys from
 * `seed`, image first_image+i, index) and writes them ASCENDING: pos_idx [N, max_pos], neg_idx [N, batch_size], padded
 * with -1; every index has i*index_offset_per_image added (batch-flattened indices); counts [N,2] = (#pos, #neg) taken. */
int abr_sample_pos_neg(const void* labels, int labels_are_int64, int N, int n, int64_t stride, int batch_size,
                       int max_pos, uint64_t seed, int first_image, int64_t index_offset_per_image,
                       int64_t* pos_idx, int64_t* neg_idx, int32_t* counts, void* stream);

/* Box-head training targets of a whole batch in three launches and NO host round trip -- what RPNPostProcessor.add_gt_proposals
 * (rpn/inference.py:53-74) + FastRCNNLossComputation.subsample (box_head/loss.py:56-120: match, label, encode, sample, cut) +
 * Pooler.convert_to_roi_format (poolers.py:73-86) do per image with a dozen small ops and two device synchronisations each:
 *   props [N,k_pre,4] decoded score-sorted boxes, keep [N,post] / n_keep [N] = abr_nms_sorted_batched's output (device);
 *   gt_ptrs / gt_label_ptrs [N] device arrays of device pointers to each image's GT boxes [G_i,4] / labels [G_i] int64, n_gt [N];
 *   candidates of image i = kept proposals then GT (Pmax = post + g_max rows per image):
 *     cand [N,Pmax,4], labels_all [N,Pmax] int64 (rows past the count = -1), regt_all [N,Pmax,4], n_cand [N];
 *   sampler (abr_sample_pos_neg on labels_all): pos_idx [N,max_pos], neg_idx [N,batch_size], counts [N,2];
 *   sampled rows, ascending candidate order per image, batch_size rows per image (rows past the number drawn: label -1, zero box):
 *     rois [N*batch_size,5] = (image, x1,y1,x2,y2), labels [N*batch_size], reg_targets [N*batch_size,4], sampled_idx [N,batch_size];
 *   obj [N*batch_size] the rows' objectness (scores [N,k_pre] for proposals, 1 for GT; obj_all [N,Pmax] scratch);
 *   pos_rows [N*batch_size] = row index where label > 0 else -1, col0 = num_classes + 4*label (or + 4 when cls_agnostic): the rows
 *   and columns of the fused predictor output that enter the box-regression loss (box_head/loss.py:166-171);
 *   n_valid [1] fp32 = total number of drawn rows (the denominator of the box-regression loss, box_head/loss.py:179). */
int abr_roi_head_targets(const float* props, const int32_t* keep, const int32_t* n_keep, int N, int k_pre, int post,
                         const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt, int g_max, float hi,
                         float lo, float wx, float wy, float ww, float wh, int batch_size, int max_pos, uint64_t seed, float* cand,
                         int64_t* labels_all, float* regt_all, int32_t* n_cand, int64_t* pos_idx, int64_t* neg_idx, int32_t* counts,
                         float* rois, int64_t* labels, float* reg_targets, int64_t* sampled_idx, float* n_valid, const float* scores,
                         float* obj_all, float* obj, int64_t* pos_rows, int64_t* col0, int num_classes, int cls_agnostic, void* stream);
/* abr_roi_head_targets for the pyramid proposal selector's output (abr_rpn_pyramid_select), csrc/box_head_fpn.hip: the proposals of image i
 * are rows [0, min(n_out[i], cap)) of the dense table rois_in [N,cap,4] with scores [N,cap] -- no keep indirection.  Everything else is
 * abr_roi_head_targets' contract with k_pre = post = cap (Pmax = cap + g_max candidates per image), in the same three launches and by the
 * same device code (csrc/roi_targets.h): given the same candidates and seed the two calls write the same bits.  An image with fewer than
 * batch_size candidates (the normal case under FPN_POST_NMS_PER_BATCH) ends in padding rows: label -1, zero box, sampled_idx -1. */
int abr_roi_head_targets_table(const float* rois_in, const float* scores, const int32_t* n_out, int N, int cap,
                               const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt, int g_max, float hi,
                               float lo, float wx, float wy, float ww, float wh, int batch_size, int max_pos, uint64_t seed, float* cand,
                               int64_t* labels_all, float* regt_all, int32_t* n_cand, int64_t* pos_idx, int64_t* neg_idx, int32_t* counts,
                               float* rois, int64_t* labels, float* reg_targets, int64_t* sampled_idx, float* n_valid, float* obj_all,
                               float* obj, int64_t* pos_rows, int64_t* col0, int num_classes, int cls_agnostic, void* stream);
/* RPN training targets of a whole batch (rpn/loss.py:66-102 per image: boxlist_iou, Matcher with low-quality matches, labels with the
 * visibility / between-thresholds discards, BoxCoder.encode) in two launches: anchors [n,4] shared by the images, gt_ptrs / vis_ptrs [N]
 * device arrays of device pointers ([G_i,4] fp32 / [n] uint8), n_gt [N]; labels [N,n] fp32 (1 / 0 / -1), reg_targets [N,n,4];
 * workspace >= N*g_max*4 bytes. */
int abr_rpn_targets_batched(const float* anchors, int n, int N, const float* const* gt_ptrs, const int32_t* n_gt, int g_max,
                            const uint8_t* const* vis_ptrs, float hi, float lo, float wx, float wy, float ww, float wh, float* labels,
                            float* reg_targets, void* workspace, int64_t workspace_bytes, void* stream);
/* RPN loss bookkeeping in one launch: pos [n_pos] / neg [n_neg] = abr_sample_pos_neg's batch-flattened, -1 padded lists, counts [n_img,2];
 * samp [n_pos+n_neg] = their concatenation, obj_flat = position of each sampled anchor's objectness logit in the fused NHWC head output
 * ([rows, Cf], anchor j -> row j / A, column j % A), pos_row / pos_col [n_pos] = row and first delta column (A + 4 (j % A)) of the
 * positives, denom [1] fp32 = number of sampled anchors (rpn/loss.py:136,146). */
int abr_rpn_loss_indices(const int64_t* pos, int n_pos, const int64_t* neg, int n_neg, const int32_t* counts, int n_img, int A, int Cf,
                         int64_t* samp, int64_t* obj_flat, int64_t* pos_row, int64_t* pos_col, float* denom, void* stream);
/* rois [N*P,5] = (i, props[i, keep[i, picks[i*P+j]]]), obj [N*P] (or NULL) = the matching scores: the P picked distillation
 * proposals per image of the source model (generalized_rcnn.py:140-158) straight from the NMS output */
int abr_gather_proposals(const float* props, const float* scores, const int32_t* keep, int N, int k_pre, int post,
                         const int64_t* picks, int P, float* rois, float* obj, void* stream);

/* =====================================================================================================
 * 6. Optimiser (solver/build.py:7-21, torch.optim.SGD semantics, one fused launch over all tensors)
 *    p,g,m flat fp32 buffers of `total` elements; seg_end[i] = exclusive end offset of tensor i;
 *    per-tensor lr[i], wd[i] (host arrays copied by the call).  m = mu*m + (g + wd*p); p -= lr*m.
 *    gscale multiplies g first (1/world_size after an RCCL sum all-reduce).
 * ===================================================================================================== */
int abr_sgd_momentum(float* p, const float* g, float* m, int64_t total, const int64_t* seg_end_dev,
                     const float* lr_dev, const float* wd_dev, int n_seg, float momentum, float gscale,
                     int first_step, void* stream);

/* =====================================================================================================
 * 7. ABR data path pixel work: uint8 HWC RGB images resident on the device.
 *    voc_abr.py:512-816 (box-crop resize, mixup blend, mosaic paste), transforms.py:64-165 (Resize, flip, ToTensor, Normalize),
 *    image_list.py:57-70 (zero-padded batch).  All results are bit-identical to the Pillow / numpy / torch-CPU originals.
 * ===================================================================================================== */
/* Pillow's 8-bit separable resampler (Image.resize).  bounds_* [out,2] int32 = (first tap, tap count), coeffs_* [out,ksize] int32 =
 * 22-bit fixed-point weights, both computed by the host exactly as Resample.c precompute_coeffs does (abr_iod_amd/data/resample.py);
 * horizontal pass first; tmp [H,OW,3] is needed when both sizes change. */
int abr_img_resample_u8(const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int32_t* bounds_h,
                        const int32_t* coeffs_h, int ksize_h, const int32_t* bounds_v, const int32_t* coeffs_v, int ksize_v,
                        uint8_t* tmp, void* stream);
/* img[y0:y0+rh, x0:x0+rw] = (uint8)(lam*img[...] + (1-lam)*crop[off_y:off_y+rh, off_x:off_x+rw]) in float64 (voc_abr.py:664-683) */
int abr_img_blend_paste_u8(uint8_t* img, int H, int W, const uint8_t* crop, int CH, int CW, int x0, int y0, int rw, int rh,
                           int off_x, int off_y, double lam, void* stream);
/* dst[dy:dy+rh, dx:dx+rw] = src[sy:sy+rh, sx:sx+rw]  (mosaic tiles, voc_abr.py:765) */
int abr_img_copy_rect_u8(uint8_t* dst, int DH, int DW, const uint8_t* src, int SH, int SW, int dx, int dy, int sx, int sy,
                         int rw, int rh, void* stream);
int abr_img_fill_u8(uint8_t* dst, int64_t n, int value, void* stream);
/* ColorJitter (transforms.py:132-150 -> torchvision.transforms.ColorJitter -> Pillow's ImageEnhance / HSV conversions), one op in place:
 * op 0 brightness, 1 contrast, 2 saturation: img = Image.blend(degenerate, img, factor) with Pillow's float32 arithmetic (degenerate = black /
 * the constant int(mean(L) + 0.5) / the pixel's L); op 3 hue: H += uint8(factor * 255) (mod 256) through Pillow's RGB <-> HSV conversions,
 * factor in [-0.5, 0.5].  scratch8: 8 bytes of device memory (used by contrast). */
int abr_img_color_jitter_u8(uint8_t* img, int H, int W, int op, double factor, void* scratch8, void* stream);
/* one [3,HP,WP] fp32 slot of the batch tensor: (optional hflip) -> /255 -> [2,1,0]*255 (to_bgr255) -> (x-mean)/std, zeros outside
 * [h,w] (transforms.py:108-165 + to_image_list).  mean/std are HOST pointers to 3 floats. */
int abr_img_normalize_to_batch(const uint8_t* src, int h, int w, int flip, int to_bgr255, const float* mean3_host,
                               const float* std3_host, float* out_slot, int HP, int WP, void* stream);

/* =====================================================================================================
 * 8. Data-parallel gradient exchange: what DistributedDataParallel's reducer does for the reference
 *    between backward and optimizer.step() (tools/train_incremental.py:231-235; reduce in maskrcnn_benchmark/engine/trainer.py:15-37),
 *    as an in-place sum all-reduce of element ranges of the FLAT fp32 gradient buffer over RCCL (csrc/comm.hip).  One process per GPU.
 *    librccl.so.1 is loaded at first use (a copy the process already holds is reused).  Rendezvous: rank 0 calls abr_comm_unique_id and
 *    distributes the 128 bytes out of band; every rank then calls abr_comm_init (collective) on its own device.
 * ===================================================================================================== */
/* RCCL's version code (ncclGetVersion), 0 when librccl cannot be loaded */
int abr_comm_rccl_version(void);
/* id128_host: 128 bytes (ncclUniqueId) */
int abr_comm_unique_id(void* id128_host);
/* *comm_out = a communicator of `world` ranks on the CURRENT device (hipSetDevice first); collective over the ranks */
int abr_comm_init(int world, int rank, const void* id128_host, void** comm_out);
/* out[0] = ranks, out[1] = this rank, out[2] = device ordinal the communicator was created on */
int abr_comm_info(void* comm, int32_t* out_host);
int abr_comm_destroy(void* comm);
/* flat[a_i : b_i) = sum over ranks, in place, for the n_ranges ranges ranges_host = {a_0, b_0, a_1, b_1, ...} (element offsets, HOST array):
 * ONE RCCL group enqueued on `stream`; returns without synchronising.  Every rank must pass the same ranges in the same order. */
int abr_allreduce_flat(void* comm, float* flat, const int64_t* ranges_host, int n_ranges, void* stream);

/* =====================================================================================================
 * 9. Mask head (MODEL.MASK_ON, MaskRCNNC4Predictor; maskrcnn_benchmark/modeling/roi_heads/mask_head/).  The two contractions (the 2x2
 *    stride-2 deconvolution as a GEMM with 4 * C_mid output columns, the 1x1 logits conv) run through abr_conv_forward / abr_conv_wgrad;
 *    these are the memory-bound kernels around them (csrc/mask.hip).  NHWC activations, fp32.
 * ===================================================================================================== */
/* rows with labels[i] > 0, in ascending order: pos_rows / pos_labels [P_max] (-1 past the count), inv [K] (position of row i in pos_rows,
 * or -1), n_pos [1] = min(count, P_max).  No host read-back: every consumer below takes the fixed-size, -1 padded lists. */
int abr_mask_compact_pos(const int64_t* labels, int K, int P_max, int64_t* pos_rows, int64_t* pos_labels, int64_t* inv, int32_t* n_pos,
                         void* stream);
/* out[p, :] = x[rows[p], :] for p < n_out (zeros where rows[p] < 0); x [n_src, row_floats], row_floats % 4 == 0.  With rows = inv of
 * abr_mask_compact_pos this is also the gather's backward: every row of the head output's gradient is written once, no atomics. */
int abr_mask_gather_rows(const float* x, const int64_t* rows, int n_src, int n_out, int64_t row_floats, float* out, void* stream);
/* project_masks_on_boxes (mask_head/loss.py:11-42) for the rows pos_rows [P_max] of the RoI table rois [K,5] (batch index, x1, y1, x2, y2):
 * the matched instance (first maximum IoU over the image's GT boxes gt_ptrs[img] [n,4]) of mask_ptrs[img] ([n,H,W] uint8 or fp32;
 * mask_dims [N,3] = n, H, W) is cropped to the box (corners rounded half to even, clamped as BinaryMaskList.crop) and resized to
 * M x M (bilinear, align_corners=False; uint8 masks truncate) -> out [P_max, M, M] fp32, zeros for padding rows. */
int abr_mask_targets(const void* const* mask_ptrs, const int32_t* mask_dims, int is_u8, const float* const* gt_ptrs, const float* rois,
                     const int64_t* pos_rows, int P_max, int K, int N, int M, float* out, void* stream);
/* y [P,h,w,4*Cm] (columns (dy*2+dx)*Cm + co: the deconvolution's GEMM) -> out [P,2h,2w,Cm] = relu(y + bias[co]) */
int abr_mask_d2s_bias_relu(const float* y, const float* bias, int P, int h, int w, int Cm, float* out, void* stream);
/* gy [P,h,w,4*Cm] = out > 0 ? g : 0 in the GEMM's column order (g, out [P,2h,2w,Cm]); the bias gradient is abr_bias_grad of gy seen as
 * [P*h*w*4, Cm] */
int abr_mask_d2s_bias_relu_backward(const float* g, const float* out, int P, int h, int w, int Cm, float* gy, void* stream);
/* mask_head/loss.py:102-128: mean over (rows with 0 < labels[p] < Kc) x MM of BCE-with-logits(logits[p, :, labels[p]], targets[p, :]);
 * logits [P,MM,ldk] (ldk % 4 == 0 >= Kc), targets [P,MM].  n_pos (device, optional): the mean's row count (NULL: P); 0 gives loss 0 and
 * zero gradients.  grad (optional) [P,MM,ldk] is written whole.  The sum is a fixed tree: two runs agree bit for bit. */
int abr_mask_loss(const float* logits, int ldk, int Kc, const int64_t* labels, const float* targets, int P, int MM, const int32_t* n_pos,
                  float* loss_out, float gscale, float* grad, void* stream);
/* mask_head/inference.py:38-45: out [D,MM] = sigmoid(logits[d, :, labels[d]]) */
int abr_mask_select_sigmoid(const float* logits, int ldk, int Kc, const int64_t* labels, int D, int MM, float* out, void* stream);
/* Masker / paste_mask_in_image (inference.py:91-159, padding 1) for all detections of one image: prob [D,M,M], boxes [D,4] xyxy ->
 * out uint8 [D,im_h,im_w] (1 where the resized mask exceeds thresh >= 0) */
int abr_mask_paste(const float* prob, const float* boxes, int D, int M, int im_h, int im_w, float thresh, uint8_t* out, void* stream);

/* =====================================================================================================
 * 10. Instance-mask evaluation (VOC box and mask AP; maskrcnn_benchmark/data/datasets/evaluation/voc/voc_eval_inst.py:89-105): the pixel
 *     counts behind masklist_iou as integer popcounts over bit-packed masks (csrc/mask_eval.hip).  Packed form of masks [n,H,W]:
 *     [n, H, Wq] 64-bit words, Wq = ceil(W / 64); bit x % 64 of word x / 64 of row y is set iff mask[i,y,x] == 1 (a 255 is not "set",
 *     as in the reference's test); the tail bits of a row's last word are zero.
 * ===================================================================================================== */
/* masks [n,H,W] uint8 (is_u8) or fp32 -> bits [n,H,Wq] */
int abr_mask_pack_bits(const void* masks, int is_u8, int n, int H, int W, uint64_t* bits, void* stream);
/* The bits of BinaryMaskList.resize((Wd,Hd)) (structures/segmentation_mask.py:113-135) of uint8 masks [n,Hs,Ws]: bilinear with
 * align_corners=False in fp32, truncated to uint8, compared with 1 -- bit for bit what torch computes on the CPU; the resized image is
 * never stored.  Equal sizes are abr_mask_pack_bits. */
int abr_mask_resize_pack_bits(const uint8_t* masks, int n, int Hs, int Ws, int Hd, int Wd, uint64_t* bits, void* stream);
/* pred_bits [P,words], gt_bits [T,words] (words = H * Wq) -> inter [P,T] = popcount(pred & gt), area_p [P], area_t [T], all int32, one
 * launch.  With pred_labels [P] and gt_labels [T] (both or neither) a pair whose labels differ gets inter = 0 and is not read.  P == 0 or
 * T == 0: success, nothing launched or written. */
int abr_mask_pair_counts(const uint64_t* pred_bits, const uint64_t* gt_bits, const int64_t* pred_labels, const int64_t* gt_labels, int P, int T,
                         int H, int W, int64_t words, int32_t* inter, int32_t* area_p, int32_t* area_t, void* stream);

/* =====================================================================================================
 * 11. COCO run-length masks (csrc/rle.hip): what pycocotools' mask_utils.decode / encode compute, restated from the format (pycocotools
 *     cannot be run where this library is built: compatibility rests on the restatement in DESIGN.md section 4 and its known answers).
 *     An RLE of an h x w mask: pixels in COLUMN-major order p = x * h + y, counts = lengths of alternating runs, the first of zeros,
 *     summing to h * w.  Compressed form: ASCII characters in [48,111]; the i-th stored value is counts[i] - counts[i-2] for i > 2 and
 *     counts[i] otherwise, 5 bits per character low bits first, 0x20 = another character follows, 0x10 of the last = sign.
 * ===================================================================================================== */
/* Decode the n instances of ONE image (all h x w) in one call.  Give EITHER bytes (uint8 [n_items], the n compressed strings
 * concatenated) OR counts (int32 [n_items], the n uncompressed count lists concatenated); offsets int64 [n+1]: instance k owns items
 * [offsets[k], offsets[k+1]).  Outputs, either or both: masks uint8 [n,h,w] row-major 0/1 (4-byte aligned); bits [n,h,ceil(w/64)] in
 * abr_mask_pack_bits' layout.  totals int64 [n]: the sum of instance k's counts -- the annotation is well formed iff totals[k] == h * w;
 * bytes that have no sum give a negative code: -1 the last token is cut short, -2 a character outside [48,111], -3 a token longer than 7
 * characters or a value outside int32, -4 a negative count.  An instance whose total is not h * w decodes to zeros.  No write lands outside
 * masks / bits / totals / workspace whatever the bytes and offsets hold (offsets are clamped into [0, n_items]).
 * workspace: abr_rle_decode_workspace_bytes(n, n_items) bytes.  n == 0: success, nothing launched. */
int64_t abr_rle_decode_workspace_bytes(int n, int64_t n_items);
int abr_rle_decode(const uint8_t* bytes, const int32_t* counts, const int64_t* offsets, int n, int64_t n_items, int h, int w, uint8_t* masks,
                   uint64_t* bits, int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream);
/* Encode n masks of one size: EITHER masks uint8 [n,h,w] (a pixel is set iff it == 1, as in abr_mask_pack_bits) OR bits [n,h,ceil(w/64)].
 * Outputs: offsets int64 [n+1] (instance k's compressed string is out_bytes[offsets[k] .. offsets[k+1])), nruns int32 [n] (its number of
 * counts), out_bytes uint8 [capacity].  Capacity protocol: offsets and nruns are ALWAYS written; the characters are written only when
 * offsets[n] <= capacity (all or nothing).  The caller reads offsets back (it needs them anyway) and, when offsets[n] > capacity, calls again
 * with at least offsets[n] bytes; capacity 0 is a pure sizing call.  workspace: abr_rle_encode_workspace_bytes(n, h, w) bytes. */
int64_t abr_rle_encode_workspace_bytes(int n, int h, int w);
int abr_rle_encode(const uint8_t* masks, const uint64_t* bits, int n, int h, int w, uint8_t* out_bytes, int64_t capacity, int64_t* offsets,
                   int32_t* nruns, void* workspace, int64_t workspace_bytes, void* stream);

/* =====================================================================================================
 * 12. Polygon instance masks (csrc/poly.hip): what pycocotools' rleFrPoly + merge + decode compute for COCO "segmentation" polygons,
 *     restated from the algorithm.  Storage of one image: coords float32 [n_vert,2] (x, y); poly_offsets int64
 *     [n_poly+1]: polygon p owns vertices [poly_offsets[p], poly_offsets[p+1]); inst_offsets int64 [n+1]: instance i owns polygons
 *     [inst_offsets[i], inst_offsets[i+1]).  An instance is the OR of its polygons; one without polygons is all zeros.
 *     Guard: a polygon with a non-finite coordinate (flag 1) or a coordinate c with |5 c| > 5 * 32768 (flag 2) contributes nothing.
 * ===================================================================================================== */
/* Rasterise the n instances of ONE image on its h x w grid.  Outputs, either or both: masks uint8 [n,h,w] row-major 0/1 (4-byte aligned);
 * bits [n,h,ceil(w/64)] in abr_mask_pack_bits' layout (the bytes are never written when only bits are asked for).  status int32 [n]: the
 * OR of the guard flags of the instance's polygons, 0 = fine.  No write lands outside masks / bits / status / workspace whatever the
 * offsets hold (they are clamped into [0, n_vert] and [0, n_poly]).  workspace: abr_poly_rasterize_workspace_bytes(n_poly, h, w) bytes,
 * 8-byte aligned (-1: bad sizes; h * w must stay below 2^31 - 64).  n == 0: success, nothing launched. */
int64_t abr_poly_rasterize_workspace_bytes(int64_t n_poly, int h, int w);
int abr_poly_rasterize(const float* coords, const int64_t* poly_offsets, const int64_t* inst_offsets, int n, int64_t n_poly, int64_t n_vert, int h,
                       int w, uint8_t* masks, uint64_t* bits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);
/* The polygon twin of abr_mask_targets (mask_head/loss.py:11-42 over PolygonList): for row pos_rows[p] of rois [K,5] (image index, xyxy),
 * the instance of its image with the first maximum IoU against gt_ptrs[img] [G,4]; its vertices through PolygonInstance.crop(box) and
 * .resize((M, M)), fl32(fl32(c - lo) * fl32(M / (hi - lo))) with the box clamped as segmentation_mask.py:251-261 and the quotient formed
 * in double; rasterised on the M x M grid.  Per-image device pointer tables coord_ptrs / poly_offset_ptrs / inst_offset_ptrs [N] and
 * dims int32 [N,5] = (instances G, polygons, vertices, image height, image width).  out float32 [P_max,M,M] of 0 / 1; rows with
 * pos_rows[p] < 0 (padding), an image index outside [0, N) or an image without instances give zeros.  M <= 64.  A guarded polygon
 * contributes nothing.  No host read-back, no allocation; P_max == 0: success, nothing launched. */
int abr_poly_mask_targets(const float* const* coord_ptrs, const int64_t* const* poly_offset_ptrs, const int64_t* const* inst_offset_ptrs,
                          const int32_t* dims, const float* const* gt_ptrs, const float* rois, const int64_t* pos_rows, int P_max, int K, int N, int M,
                          float* out, void* stream);

/* =====================================================================================================
 * 13. COCO detection scoring (csrc/coco_eval.hip, csrc/coco_oks.hip): the per-image work of pycocotools' COCOeval -- computeIoU / computeOks
 *     and evaluateImg -- restated
 *     from the protocol.  A GROUP is one (image, category) pair: its detections in rank order (score descending,
 *     stable, at most maxDets) and its ground truths in file order.  The groups of a batch lie flat: group k owns detections
 *     [det_off[k], det_off[k+1]), ground truths [gt_off[k], gt_off[k+1]) and the row-major D_k x G_k float64 IoU matrix at iou_off[k]
 *     (iou_off[k+1] - iou_off[k] == D_k * G_k); all three tables int64 [n_groups+1].  Every call is ONE launch for the batch.
 * ===================================================================================================== */
#define ABR_COCO_MATCH_MAX_GT 128
/* the ground truths per group abr_coco_match holds (ABR_COCO_MATCH_MAX_GT) */
int abr_coco_match_max_gt(void);
/* bbIou: det [D_total,4], gt [G_total,4] float64 xywh, gt_crowd uint8 [G_total] -> iou float64 [total], total = iou_off[n_groups].
 * area = w * h (no + 1); a pair whose intersection has no positive width or height gets 0; else i / (a_d + a_g - i), or i / a_d when the
 * ground truth is a crowd.  One rounding per operation. */
int abr_coco_box_iou(const double* det, const double* gt, const uint8_t* gt_crowd, const int64_t* det_off, const int64_t* gt_off,
                     const int64_t* iou_off, int n_groups, int64_t total, double* iou, void* stream);
/* The counts of abr_mask_pair_counts for one image (inter [P,T], area_p [P], area_t [T]) and gt_crowd uint8 [T] -> iou float64 [P,T]:
 * inter / (area_p + area_t - inter), or inter / area_p for a crowd column; 0 where inter == 0.  P == 0 or T == 0: nothing launched. */
int abr_coco_mask_iou(const int32_t* inter, const int32_t* area_p, const int32_t* area_t, const uint8_t* gt_crowd, int P, int T, double* iou,
                      void* stream);
/* evaluateImg for every group, all A area ranges (area_rng float64 [A,2], both ends inclusive) and all T IoU thresholds (thrs float64 [T],
 * used as given) at once; A <= 8 and A * T <= 64.  det_area [D_total], gt_area [G_total] float64.  Outputs: dt_gt int32 [A,T,D_total]: the
 * matched ground truth's ROW in its group, -1 = unmatched; dt_ig uint8 [A,T,D_total]: the detection is ignored; gt_ig uint8 [A,G_total]:
 * the ground truth is ignored (a crowd, or its area outside the range).  A group with more than ABR_COCO_MATCH_MAX_GT ground truths is
 * NOT scored: none of its outputs is written and *n_over (device int32, zeroed by the caller) counts it -- the caller scores it on the host. */
int abr_coco_match(const double* iou, const int64_t* iou_off, const int64_t* det_off, const int64_t* gt_off, const double* det_area,
                   const double* gt_area, const uint8_t* gt_crowd, int n_groups, int64_t d_total, int64_t g_total, const double* area_rng, int A,
                   const double* thrs, int T, int32_t* dt_gt, uint8_t* dt_ig, uint8_t* gt_ig, int32_t* n_over, void* stream);
/* abr_coco_match with the protocol's `ignore` flag beside the crowd flag: gt_ignore uint8 [G_total]; a ground truth is ignored when
 * gt_ignore is set or its area is outside the range, and gt_crowd alone lets a matched ground truth be matched again.  Keypoints:
 * gt_ignore = crowd or no labelled keypoint.  abr_coco_match is this entry with gt_ignore = gt_crowd. */
int abr_coco_match_ig(const double* iou, const int64_t* iou_off, const int64_t* det_off, const int64_t* gt_off, const double* det_area,
                      const double* gt_area, const uint8_t* gt_crowd, const uint8_t* gt_ignore, int n_groups, int64_t d_total, int64_t g_total,
                      const double* area_rng, int A, const double* thrs, int T, int32_t* dt_gt, uint8_t* dt_ig, uint8_t* gt_ig, int32_t* n_over,
                      void* stream);
/* computeOks (csrc/coco_oks.hip): det_kp [D_total,K,3], gt_kp [G_total,K,3] float64 (x, y, visibility), gt_box [G_total,4] xywh, gt_area
 * [G_total], var [K] = (2 sigma_k)^2 -> oks float64 [total] in abr_coco_box_iou's layout.  With k1 = the ground truth's keypoints of
 * visibility > 0: k1 > 0: the mean over those of exp(-((xd-xg)^2 + (yd-yg)^2) / var_k / (area + 2^-52) / 2); k1 == 0: the mean over all K
 * with the distances to the box doubled about itself ([x - w, x + 2w] x [y - h, y + 2h]) in place of the differences.  One rounding per
 * operation, the sum serial in keypoint order; crowds get no special value.  Any K >= 1, no cap on D or G. */
int abr_coco_oks(const double* det_kp, const double* gt_kp, const double* gt_box, const double* gt_area, const double* var, int K,
                 const int64_t* det_off, const int64_t* gt_off, const int64_t* iou_off, int n_groups, int64_t total, double* oks, void* stream);

/* =====================================================================================================
 * 14. Keypoint head (MODEL.KEYPOINT_ON; csrc/keypoint.hip; maskrcnn_benchmark/modeling/roi_heads/keypoint_head/).  The low-resolution heat
 *     maps are PLANAR [P,Kp,H,W], Kp = K rounded up to a multiple of 4; channels k >= K are padding.  fp32 arithmetic, no read-back, no
 *     floating-point atomics: every sum has a fixed order and two runs agree bit for bit.
 * ===================================================================================================== */
/* keypoint_head/loss.py:39-143 + structures/keypoint.py:154-188 for the whole batch in one launch.  rois [R,5] (image index, xyxy) and
 * labels [R] are the box head's sampled set.  A row is kept when labels > 0 and the instance of its image with the first maximum IoU
 * (gt_ptrs[img] [n_gt[img],4]) has a keypoint (kp_ptrs[img] [n_gt[img],K,3] = x, y, visibility) that is visible (> 0) and inside that
 * instance's box (inclusive).  Kept rows in ascending order: pos_rows [P_max] int64 (-1 padded; rows past P_max are dropped), inv [R] =
 * position in pos_rows or -1, *n_pos.  tgt [P_max,K] int64 = y * M + x with x = floor((kx - x1) * ((1 / (x2 - x1)) * M)) in fp32, torch's order (kx == x2
 * gives M - 1; the same for y), 0 where valid [P_max,K] uint8 is 0: the keypoint is not visible or leaves [0, M) on an axis (inf and NaN
 * of a zero-width RoI included).  *n_valid = the number of valid entries.  An image index outside [0, N) or n_gt[img] <= 0: row dropped. */
int abr_kp_select_targets(const float* rois, const int64_t* labels, int R, const float* const* gt_ptrs, const float* const* kp_ptrs,
                          const int32_t* n_gt, int N, int K, int M, int P_max, int64_t* pos_rows, int64_t* inv, int32_t* n_pos, int64_t* tgt,
                          uint8_t* valid, int32_t* n_valid, void* stream);
/* ConvTranspose2d(C, K, 4, stride 2, padding 1) behind its GEMM: y [P,h,w,16*Kp] (columns (ky*4+kx)*Kp + k) -> out [P,Kp,2h,2w] planar,
 * out[p,k,oy,ox] = bias[k] + sum of y[p,iy,ix,(ky,kx,k)] over the at most 2 x 2 taps with oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx, added
 * in (ky, kx) order; bias [K]; the planes k >= K are written as zeros. */
int abr_kp_deconv_fold(const float* y, const float* bias, int P, int h, int w, int K, float* out, void* stream);
/* the fold's exact adjoint: g [P,Kp,2h,2w] -> gy [P,h,w,16*Kp], zeros for taps outside the map and for columns k >= K */
int abr_kp_deconv_unfold(const float* g, int P, int h, int w, int K, float* gy, void* stream);
/* interpolate(scale_factor=2, mode="bilinear", align_corners=False): x [P,Kp,H,W] planar -> out [P,K,2H,2W] */
int abr_kp_upsample2x(const float* x, int P, int K, int H, int W, float* out, void* stream);
/* the largest H * W abr_kp_loss and Hm * Wm abr_kp_decode stage in LDS (4096 floats, 16 KB) */
int abr_kp_loss_max_plane(void);
/* keypoint_head/loss.py:145-169 on the low-resolution maps: the 2x bilinear upsampling and F.cross_entropy over the 4 H W upsampled logits
 * of every row with valid[p,k] != 0, mean over *n_valid rows (device int32; 0 gives loss 0 and zero gradients).  x [P,Kp,H,W], tgt / valid
 * [P,K] index the UPSAMPLED map (a target outside [0, 4 H W) makes its row invalid).  grad (optional) [P,Kp,H,W] is written whole: the
 * gradient with respect to x, times gscale, zeros for invalid rows and padding channels; row_sum (optional, with grad) [P,Kp] = each
 * plane's gradient sum (abr_bias_grad over it is the deconvolution's bias gradient).  H * W <= abr_kp_loss_max_plane(), P * Kp <= 65536. */
int abr_kp_loss(const float* x, int P, int K, int H, int W, const int64_t* tgt, const uint8_t* valid, const int32_t* n_valid, float gscale,
                float* loss_out, float* grad, float* row_sum, void* stream);
/* keypoint_head/inference.py:40-94 on the device.  maps: plane (d, k) at maps + d * stride_d + k * stride_k, Hm x Wm contiguous; boxes
 * [D,4] xyxy.  Each plane is resized to ceil(max(w, 1)) x ceil(max(h, 1)) by the bicubic rule (Keys' kernel, a = -0.75, source coordinate
 * (d + 0.5) src / dst - 0.5, replicated borders, no antialiasing) and its first maximum in row-major order is taken (the lowest index among
 * equal values; NaN values never win, a plane without a value above -inf gives index 0).  xy [D,K,3] = ((x_int + 0.5) w / ceil(w) + x1,
 * the same for y, 1); logit [D,K] = the resized value there.  The grid's sides are clamped to 8192.  Hm * Wm <= abr_kp_loss_max_plane(). */
int abr_kp_decode(const float* maps, int64_t stride_d, int64_t stride_k, const float* boxes, int D, int K, int Hm, int Wm, float* xy,
                  float* logit, void* stream);

/* =====================================================================================================
 * 15. Proposal recall (csrc/proposal_recall.hip; evaluation/coco/coco_eval.py: evaluate_box_proposals, restated: DESIGN.md section 4).
 *     Flat as in section 13: image k owns proposals [prop_off[k], prop_off[k+1]) and ground truths [gt_off[k], gt_off[k+1]), both tables
 *     int64 [n_images+1].  A CELL is one (image, limit, area range).
 * ===================================================================================================== */
#define ABR_PROPOSAL_COVER_MAX_PROP 1024
/* the proposals per image abr_proposal_cover holds (ABR_PROPOSAL_COVER_MAX_PROP); ground truths: ABR_COCO_MATCH_MAX_GT */
int abr_proposal_cover_max_prop(void);
/* The greedy cover of every cell in ONE launch.  prop float32 [p_total,4] xyxy in rank order (objectness descending, stable) at the
 * original image size, 16-byte aligned; gt float32 [g_total,4] xyxy (non-crowd only), 16-byte aligned; gt_area float32 [g_total];
 * area_rng float32 [A,2], both ends inclusive, A <= 8; limits int32 [L], L <= 4; thrs float32 [T], T <= 16, used as given.
 * All of these are DEVICE pointers, so the entry cannot check their values: limits[l] < 1 makes the cells of that limit empty (all -1),
 * and boxes must have x2 >= x1 and y2 >= y1 -- two boxes of +1-area zero have the overlap 0 / 0, which no round can select (a ground
 * truth left with nothing else records -1, where the reference's loop fails its assertion).
 * A cell takes the image's first min(P, limits[l]) proposals and its ground truths with lo <= gt_area <= hi (G_valid of them, file order).
 * IoU = boxlist_iou's float32 arithmetic (area = (x2 - x1 + 1) * (y2 - y1 + 1), wh = max(min(rb) - max(lt) + 1, 0), inter / (a_p + a_g -
 * inter)), one rounding per operation.  min(P, G_valid) rounds: the largest remaining overlap (ties: the lowest ground truth, then the
 * lowest proposal rank) is recorded and its proposal and ground truth retire.
 * Outputs: overlaps float32 [L,A,g_total]: of an image's segment the first G_valid slots hold the recorded values in round order, then
 * zeros; the remaining slots -1; a cell without proposals or without a ground truth in range is all -1.  hits int32 [L,A,T]: the number of
 * slots >= 0 with overlap >= thrs[t], added with integer atomics; num_pos int32 [A]: ground truths in range over all images that have one
 * (with or without proposals), added likewise; hits, num_pos and *n_over are zeroed by the caller.
 * An image with more than ABR_PROPOSAL_COVER_MAX_PROP proposals or more than ABR_COCO_MATCH_MAX_GT ground truths is NOT scored: none of
 * its outputs is written or counted and *n_over counts it once -- the caller scores it on the host.  n_images == 0 or g_total == 0:
 * success, nothing launched. */
int abr_proposal_cover(const float* prop, const float* gt, const float* gt_area, const int64_t* prop_off, const int64_t* gt_off, int n_images,
                       int64_t p_total, int64_t g_total, const float* area_rng, int A, const int32_t* limits, int L, const float* thrs, int T,
                       float* overlaps, int32_t* hits, int32_t* num_pos, int32_t* n_over, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ABR_IOD_HIP_H */
