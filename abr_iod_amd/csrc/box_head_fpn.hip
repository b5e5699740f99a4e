// The FPN box head's glue (modeling/roi_heads/box_head/fpn_box_head.py).  Its contractions -- fc6, fc7, the fused predictor and their
// gradients -- are the conv library's; what the library could not do is here:
//   abr_roi_head_targets_table  box-head training targets straight from the pyramid proposal selector's table (abr_rpn_pyramid_select:
//                               rois [N,cap,4], scores [N,cap], n_out [N]) -- the device code of abr_roi_head_targets (roi_targets.h) with a
//                               dense candidate fetch instead of the NMS keep lists;
//   abr_h3_amax_max             one fresh amax word = the largest of L existing ones: the upper bound the multi-level Pooler tags its
//                               output with (a pooled value is an average of bilinear samples of ONE of the L maps).
#include "common.h"
#include "roi_targets.h"

namespace {

struct AmaxWords {
    const unsigned long long* word[ABR_MAX_PYRAMID_LEVELS];
    unsigned epoch[ABR_MAX_PYRAMID_LEVELS];
};

// One wave.  Lane l < L reads word l; a word that no longer carries its epoch makes the result unknowable: nothing is written then, the
// output word keeps an older epoch and its reader raises ABR_H3_FLAG_STALE exactly as it would have on the level's own word.  The bits of
// non-negative floats (and of +inf / NaN, which sort above them) order as unsigned integers, so the maximum of the bits is the bits of the
// maximum.  The write is the protocol's: one 64-bit atomic max, a later epoch always wins (common.h).
__global__ __launch_bounds__(64) void h3_amax_max_kernel(const AmaxWords in, int L, unsigned long long* __restrict__ out, unsigned epoch) {
    const int l = threadIdx.x;
    unsigned bits = 0u, stale = 0u;
    if (l < L) {
        bits = abr::h3_amax_load(in.word[l], in.epoch[l]);
        // (0xFFFFFFFF is h3_amax_load's "stale" and no value an emitter can write: every emitter hands over |x|'s bits, sign bit clear)
        stale = bits == 0xFFFFFFFFu ? 1u : 0u;
        if (stale) bits = 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bits = max(bits, (unsigned)__shfl_xor((int)bits, o, 64));
        stale |= (unsigned)__shfl_xor((int)stale, o, 64);
    }
    if (l == 0 && !stale) atomicMax(out, ((unsigned long long)epoch << 32) | bits);
}

}  // namespace

extern "C" int abr_h3_amax_max(const uint64_t* const* words, const uint32_t* epochs, int L, uint64_t* out_word, uint32_t out_epoch,
                               void* stream) {
    ABR_REQUIRE(L >= 1 && L <= ABR_MAX_PYRAMID_LEVELS, "h3_amax_max: %d levels, need 1 .. %d", L, ABR_MAX_PYRAMID_LEVELS);
    ABR_REQUIRE(words && epochs && out_word, "h3_amax_max: null pointer");
    AmaxWords in;
    for (int l = 0; l < ABR_MAX_PYRAMID_LEVELS; l++) {
        in.word[l] = nullptr;
        in.epoch[l] = 0;
    }
    for (int l = 0; l < L; l++) {
        ABR_REQUIRE(words[l], "h3_amax_max: level %d has no amax word", l);
        ABR_REQUIRE(reinterpret_cast<const void*>(words[l]) != reinterpret_cast<const void*>(out_word), "h3_amax_max: the output word is level %d's", l);
        in.word[l] = reinterpret_cast<const unsigned long long*>(words[l]);
        in.epoch[l] = epochs[l];
    }
    h3_amax_max_kernel<<<1, 64, 0, abr::as_stream(stream)>>>(in, L, reinterpret_cast<unsigned long long*>(out_word), out_epoch);
    ABR_CHECK_LAUNCH("h3_amax_max");
    return ABR_OK;
}

extern "C" int abr_roi_head_targets_table(const float* rois_in, const float* scores, const int32_t* n_out, int N, int cap,
                                          const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt, int g_max,
                                          float hi, float lo, float wx, float wy, float ww, float wh, int batch_size, int max_pos,
                                          uint64_t seed, float* cand, int64_t* labels_all, float* regt_all, int32_t* n_cand,
                                          int64_t* pos_idx, int64_t* neg_idx, int32_t* counts, float* rois, int64_t* labels,
                                          float* reg_targets, int64_t* sampled_idx, float* n_valid, float* obj_all, float* obj,
                                          int64_t* pos_rows, int64_t* col0, int num_classes, int cls_agnostic, void* stream) {
    ABR_REQUIRE(N > 0 && cap > 0 && g_max > 0 && batch_size > 0 && max_pos >= 0 && max_pos <= batch_size, "roi_head_targets_table: bad sizes");
    const abr::roi_targets::Outputs o{cand, labels_all, regt_all, n_cand, pos_idx, neg_idx, counts, rois, labels, reg_targets, sampled_idx, n_valid,
                                      obj_all, obj, pos_rows, col0};
    ABR_REQUIRE(rois_in && scores && n_out && gt_ptrs && gt_label_ptrs && n_gt && o.complete(), "roi_head_targets_table: null pointer");
    const abr::roi_targets::TableFetch f{rois_in, scores, n_out, cap};
    return abr::roi_targets::run("roi_head_targets_table", f, N, cap + g_max, gt_ptrs, gt_label_ptrs, n_gt, hi, lo, wx, wy, ww, wh, batch_size,
                                 max_pos, seed, o, num_classes, cls_agnostic, stream);
}
