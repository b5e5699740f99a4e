// RetinaNet's test-time post-processor over a feature pyramid, on the device from the head's logits to the detections of every image.
//
// Reference: maskrcnn_benchmark/modeling/rpn/retinanet/inference.py.  Per image and level (:73-123) a boolean index, a topk, a nonzero, two
// gathers, a decode and a clip; then per image (:131-174) a loop over every class with a nonzero, an index and an NMS with a host loop, and a
// kthvalue through the CPU: for 2 images, 5 levels and 80 classes several hundred launches and hundreds of host synchronisations.  Here, with
// S = N * L (image, level) segments, segment s = i * L + l:
//
//   abr_retina_detect   1 memset + 4 launches, whatever N, L and the class count are; nothing is read back
//     1. histogram (grid: slices x S): every logit of the level once; the CANDIDATES are those whose sigmoid (abr::sigmoid_key's float) exceeds
//        the threshold; a histogram of the candidates' top 12 key bits per segment (LDS per workgroup, flushed with integer atomics).
//     2. partition (grid: slices x S): every workgroup reads the candidate count and, when it exceeds k = PRE_NMS_TOP_N, the bin b1 holding the
//        k-th key off the histogram; words (abr::rank_word: key << 32 | ~flat index) above the bin are SURVIVORS (fewer than k), words inside
//        it go to the bin list; with at most k candidates all of them are survivors.  Appended per segment by a counting pass, one reservation
//        per workgroup and a writing pass.  From here on the cost follows the number of candidates, not of logits.
//     3. select + sort + decode (one 1024-thread workgroup per segment): the (k - #survivors)-th largest word of the bin list by five more radix
//        levels (abr::kth_word; words are unique, so the cut is exact whichever workgroup won which atomic), a bitonic sort in LDS -- descending
//        score, equal scores by ascending flat index loc * A * C + a * C + c -- then anchor = flat / C, label = flat % C + 1, abr::box_decode,
//        abr::box_clip, remove_small_boxes and a stable compaction in rank order (abr::compact_pos) into the segment's rows of scratch.
//     4. classes + NMS + cut (one 1024-thread workgroup per image): the image's at most L * k candidates get a CLASS WORD
//        (~label : 19 | score bits : 32 | ~position : 13, position p = level * k + rank) and are sorted once in LDS: class by class, inside a class
//        by descending score, equal scores by ascending position.  A class is then one contiguous run, and greedy NMS (abr::nms_suppresses, the
//        rule of nms.hip) runs per run, one wave per run, the runs dealt round-robin to the 16 waves -- boxes of different labels never meet.
//        The survivors, already in the reference's output order (class 1's by descending score, then class 2's, ...), become rank words; when
//        more than detections_per_img remain abr::kth_word finds the detections_per_img-th largest and every survivor whose SCORE reaches that
//        word's score is emitted (ties at the cut all kept, order unchanged) through the same stable compaction.
//     LDS of kernel 4 (dynamic): p2 words (p2 = L * k rounded up to a power of two, <= 8192: 64 KB) + p2 flag bytes + 16 KB histogram.
//     Hence L * PRE_NMS_TOP_N <= 8192 (abr_retina_max_candidates) and PRE_NMS_TOP_N <= 2048 (abr_rpn_pyramid_max_k); the defaults need 5 x 1000.
//     Scratch (per stream, from the pool): [histograms S x 4096][counters S][survivors S x 2048 words][boxes, scores, labels S x k][counts S]
//     [bin lists: a word per logit].  Histograms and counters are zeroed by the call itself, everything else is written before it is read.
#include <algorithm>

#include "box_math.h"
#include "rank_select.h"

namespace {

using abr::find_bin_from_top;

constexpr int MAXL = ABR_MAX_PYRAMID_LEVELS;
constexpr int KT = 256;        // threads of the chip-wide kernels
constexpr int TT = 1024;       // threads of the per-segment and per-image kernels
constexpr int HB = 4096;       // bins of a 12-bit level
constexpr int KCAP = 2048;     // most candidates ranked per segment (the in-LDS sort)
constexpr int ICAP = 8192;     // most candidates per image (the in-LDS sort of kernel 4; 13 position bits of the class word)
constexpr int G = 64;          // slices per segment
constexpr int LABEL_BITS = 19, POS_BITS = 13;
constexpr unsigned LABEL_MASK = (1u << LABEL_BITS) - 1, POS_MASK = (1u << POS_BITS) - 1;

struct RetLevels {             // by value in the kernel arguments: no device-side table
    const float* cls[MAXL];        // [N, nloc, ldc]: columns 0 .. A*C-1 the logits, a * C + c
    const float* reg[MAXL];        // [N, nloc, ldr]: columns 4a .. 4a+3 the deltas of anchor a
    const float* anchors[MAXL];    // [nloc * A, 4]
    int nloc[MAXL], ldc[MAXL], ldr[MAXL], k[MAXL], per[MAXL];
    long long n[MAXL];             // nloc * A * C logits (fits int32)
    long long off[MAXL];           // offset of the level's bin lists [N, n] in scratch
};
struct RetCnt { int surv, bin; };

__device__ __forceinline__ unsigned class_label(unsigned long long w) { return LABEL_MASK - (unsigned)(w >> (32 + POS_BITS)); }
__device__ __forceinline__ unsigned class_key(unsigned long long w) { return (unsigned)(w >> POS_BITS); }
__device__ __forceinline__ unsigned class_pos(unsigned long long w) { return ~(unsigned)w & POS_MASK; }

// ------------------------------------------------------------------------------------------------------------------- candidates
__global__ __launch_bounds__(KT) void ret_hist_kernel(RetLevels lv, int L, int AC, float thr, int* __restrict__ hist) {
    __shared__ int lh[HB];
    const int seg = blockIdx.y, img = seg / L, l = seg % L;
    const int n = (int)lv.n[l], ldc = lv.ldc[l], per = lv.per[l];
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    if (j0 >= n) return;
    for (int i = threadIdx.x; i < HB; i += KT) lh[i] = 0;
    __syncthreads();
    const float* base = lv.cls[l] + (size_t)img * lv.nloc[l] * ldc;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = abr::sigmoid_key(base[(size_t)(j / AC) * ldc + (j % AC)]);
        if (__uint_as_float(key) > thr) atomicAdd(&lh[key >> 20], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HB; i += KT)
        if (lh[i]) atomicAdd(&hist[(size_t)seg * HB + i], lh[i]);
}

__global__ __launch_bounds__(KT) void ret_partition_kernel(RetLevels lv, int L, int AC, float thr, const int* __restrict__ hist,
                                                           unsigned long long* __restrict__ surv_all, unsigned long long* __restrict__ bin_all,
                                                           RetCnt* __restrict__ cnt_all) {
    __shared__ int h[HB];
    __shared__ int s_bin, s_krem, s_total, n_s, n_c, base_s, base_c;
    const int seg = blockIdx.y, img = seg / L, l = seg % L;
    const int n = (int)lv.n[l], k = lv.k[l], ldc = lv.ldc[l], per = lv.per[l];
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    if (j0 >= n) return;
    if (threadIdx.x == 0) { s_krem = k; s_bin = 0; s_total = 0; n_s = 0; n_c = 0; }
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < HB; i += KT) {
        const int v = hist[(size_t)seg * HB + i];
        h[i] = v;
        mine += v;
    }
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (s_total == 0) return;          // no candidate in the segment
    int b1 = -1;                       // at most k candidates: every one survives
    if (s_total > k) {
        find_bin_from_top(h, HB, &s_bin, &s_krem);
        __syncthreads();
        b1 = s_bin;
    }
    const float* base = lv.cls[l] + (size_t)img * lv.nloc[l] * ldc;
    int my_s = 0, my_c = 0;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = abr::sigmoid_key(base[(size_t)(j / AC) * ldc + (j % AC)]);
        if (__uint_as_float(key) > thr) {
            const int bin = (int)(key >> 20);
            my_s += bin > b1;
            my_c += bin == b1;
        }
    }
    if (my_s) atomicAdd(&n_s, my_s);
    if (my_c) atomicAdd(&n_c, my_c);
    __syncthreads();
    if (threadIdx.x == 0) {
        base_s = n_s ? atomicAdd(&cnt_all[seg].surv, n_s) : 0;
        base_c = n_c ? atomicAdd(&cnt_all[seg].bin, n_c) : 0;
        n_s = 0;
        n_c = 0;
    }
    __syncthreads();
    unsigned long long* surv = surv_all + (size_t)seg * KCAP;
    unsigned long long* binl = bin_all + lv.off[l] + (size_t)img * n;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = abr::sigmoid_key(base[(size_t)(j / AC) * ldc + (j % AC)]);
        if (!(__uint_as_float(key) > thr)) continue;
        const int bin = (int)(key >> 20);
        const unsigned long long w = abr::rank_word(key, (unsigned)j);
        if (bin > b1) {
            const int pos = base_s + atomicAdd(&n_s, 1);
            if (pos < KCAP) surv[pos] = w;     // (at most k <= KCAP survivors by construction)
        } else if (bin == b1) {
            const int pos = base_c + atomicAdd(&n_c, 1);
            if (pos < n) binl[pos] = w;        // (at most n: the region holds n words)
        }
    }
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(TT) void ret_select_decode_kernel(RetLevels lv, int L, int A, int C, int K, const unsigned long long* __restrict__ surv_all,
                                                               const unsigned long long* __restrict__ bin_all, const RetCnt* __restrict__ cnt_all,
                                                               const int32_t* __restrict__ img_hw, float wx, float wy, float ww, float wh, float min_size,
                                                               float* __restrict__ boxes, float* __restrict__ scores, int32_t* __restrict__ labels,
                                                               int32_t* __restrict__ counts) {
    __shared__ int h[HB];
    __shared__ unsigned long long buf[KCAP];
    __shared__ int s_wave[TT / 64];
    __shared__ int s_bin, s_krem, s_fill, s_base;
    const int seg = blockIdx.x, i = seg / L, l = seg % L;
    const int n = (int)lv.n[l], k = lv.k[l];
    const int nsurv = min(cnt_all[seg].surv, k), nbin = min(cnt_all[seg].bin, n);
    const unsigned long long* surv = surv_all + (size_t)seg * KCAP;
    const unsigned long long* binl = bin_all + lv.off[l] + (size_t)i * n;
    const int want = min(k - nsurv, nbin);        // > 0 exactly when the segment has more than k candidates
    const int m = nsurv + want;                   // min(#candidates, k)
    int p2 = 2;
    while (p2 < m) p2 <<= 1;
    for (int t = threadIdx.x; t < p2; t += TT) buf[t] = t < nsurv ? surv[t] : 0ull;    // padding sorts last
    if (threadIdx.x == 0) { s_fill = 0; s_base = 0; }
    __syncthreads();
    if (want > 0) {
        const unsigned long long thrw = abr::kth_word(binl, nbin, want, 1, binl[0] >> 52, h, &s_bin, &s_krem);
        for (int j = threadIdx.x; j < nbin; j += TT) {
            const unsigned long long w = binl[j];
            if (w >= thrw) {
                const int pos = nsurv + atomicAdd(&s_fill, 1);
                if (pos < m) buf[pos] = w;
            }
        }
        __syncthreads();
    }
    abr::bitonic_desc<TT>(buf, p2);
    const int AC = A * C, nloc = lv.nloc[l], ldr = lv.ldr[l];
    const float* reg = lv.reg[l] + (size_t)i * nloc * ldr;
    const float4* anchors = reinterpret_cast<const float4*>(lv.anchors[l]);
    float4* bo = reinterpret_cast<float4*>(boxes) + (size_t)seg * K;
    float* so = scores + (size_t)seg * K;
    int32_t* lo = labels + (size_t)seg * K;
    for (int c0 = 0; c0 < m; c0 += TT) {
        const int t = c0 + threadIdx.x;
        bool keep = false;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        int lab = 0;
        if (t < m) {
            const unsigned long long w = buf[t];
            const int flat = (int)abr::rank_word_index(w);
            sc = __uint_as_float(abr::rank_word_key(w));
            const int loc = flat / AC, col = flat % AC, a = col / C;
            lab = col % C + 1;
            o = abr::box_decode(anchors[(size_t)loc * A + a], reg + (size_t)loc * ldr + 4 * a, wx, wy, ww, wh);
            o = abr::box_clip(o, (float)(img_hw[2 * i + 1] - 1), (float)(img_hw[2 * i] - 1));
            // boxlist_ops.py:34-48 remove_small_boxes; min_size <= 0 keeps every row
            keep = min_size <= 0.f || ((o.z - o.x + 1 >= min_size) && (o.w - o.y + 1 >= min_size));
        }
        const int pos = abr::compact_pos<TT>(keep, s_wave, &s_base);
        if (keep) {
            bo[pos] = o;
            so[pos] = sc;
            lo[pos] = lab;
        }
    }
    if (threadIdx.x == 0) counts[seg] = s_base;
}

// ------------------------------------------------------------------------------------------------------------------- per image
// lower bound of the first position in the sorted class words buf[lo .. hi) whose label differs from `lab` (labels ascend along the array)
__device__ __forceinline__ int run_end(const unsigned long long* buf, int lo, int hi, unsigned lab) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (class_label(buf[mid]) == lab) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TT) void ret_image_kernel(int L, int K, int p2, float nms_thr, int det_per_img, int cap, const float* __restrict__ seg_boxes,
                                                       const float* __restrict__ seg_scores, const int32_t* __restrict__ seg_labels,
                                                       const int32_t* __restrict__ seg_counts, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                       int64_t* __restrict__ out_labels, int32_t* __restrict__ n_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* buf = reinterpret_cast<unsigned long long*>(smem);            // [p2] class words, then rank words
    int* h = reinterpret_cast<int*>(smem + (size_t)p2 * 8);                            // [HB]
    int* s_wave = h + HB;                                                              // [TT / 64]
    int* s_misc = s_wave + TT / 64;                                                    // [4]: bin, krem, base, total
    volatile unsigned char* dead = reinterpret_cast<volatile unsigned char*>(s_misc + 4);   // [p2] suppressed flags
    const int i = blockIdx.x, per_img = L * K;
    const float4* bx = reinterpret_cast<const float4*>(seg_boxes) + (size_t)i * per_img;
    const float* sc = seg_scores + (size_t)i * per_img;
    const int32_t* lb = seg_labels + (size_t)i * per_img;
    if (threadIdx.x < 4) s_misc[threadIdx.x] = 0;
    int mine = 0;
    for (int p = threadIdx.x; p < p2; p += TT) {
        unsigned long long w = 0ull;
        if (p < per_img && p % K < min(seg_counts[i * L + p / K], K)) {
            w = ((unsigned long long)(LABEL_MASK - (unsigned)lb[p]) << (32 + POS_BITS)) | ((unsigned long long)__float_as_uint(sc[p]) << POS_BITS) |
                (~(unsigned)p & POS_MASK);
            mine++;
        }
        buf[p] = w;
        dead[p] = 0;
    }
    __syncthreads();
    if (mine) atomicAdd(&s_misc[3], mine);
    abr::bitonic_desc<TT>(buf, p2);
    const int M = s_misc[3];           // the class words are buf[0 .. M): label ascending, score descending, position ascending
    // greedy NMS per class run, run r by wave r % 16; every wave walks the run boundaries itself
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int s = 0, r = 0;
        while (s < M) {
            const int e = run_end(buf, s + 1, M, class_label(buf[s]));
            if (r % (TT / 64) == wave) {
                for (int a = s; a < e; a++) {
                    if (dead[a]) continue;
                    const float4 A4 = bx[class_pos(buf[a])];
                    const float area = (A4.z - A4.x + 1) * (A4.w - A4.y + 1);
                    for (int b = a + 1 + lane; b < e; b += 64)
                        if (!dead[b] && abr::nms_suppresses(A4, area, bx[class_pos(buf[b])], nms_thr, 0)) dead[b] = 1;
                    __builtin_amdgcn_wave_barrier();
                }
            }
            s = e;
            r++;
        }
    }
    __syncthreads();
    // survivors -> rank words in place (array order = output order), then the exact detections_per_img-th largest score
    int live = 0;
    for (int p = threadIdx.x; p < p2; p += TT) {
        const unsigned long long w = buf[p];
        const bool ok = p < M && !dead[p];
        buf[p] = ok ? abr::rank_word(class_key(w), class_pos(w)) : 0ull;
        live += ok;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_misc[3] = 0;
    __syncthreads();
    if (live) atomicAdd(&s_misc[3], live);
    __syncthreads();
    const int total = s_misc[3];
    unsigned cut = 0u;                 // every score key is > 0
    if (det_per_img > 0 && total > det_per_img)
        cut = abr::rank_word_key(abr::kth_word(buf, M, det_per_img, 0, 0ull, h, &s_misc[0], &s_misc[1]));
    __syncthreads();
    float4* bo = reinterpret_cast<float4*>(out_boxes) + (size_t)i * cap;
    float* so = out_scores + (size_t)i * cap;
    int64_t* lo = out_labels + (size_t)i * cap;
    for (int c0 = 0; c0 < M; c0 += TT) {
        const int p = c0 + threadIdx.x;
        const unsigned long long w = p < M ? buf[p] : 0ull;
        const bool take = w != 0ull && abr::rank_word_key(w) >= cut;
        const int pos = abr::compact_pos<TT>(take, s_wave, &s_misc[2]);
        if (take && pos < cap) {
            const int g = (int)abr::rank_word_index(w);
            bo[pos] = bx[g];
            so[pos] = __uint_as_float(abr::rank_word_key(w));
            lo[pos] = (int64_t)lb[g];
        }
    }
    __syncthreads();
    const int count = min(s_misc[2], cap);
    if (threadIdx.x == 0) n_out[i] = count;
    for (int r = count + threadIdx.x; r < cap; r += TT) {
        bo[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        so[r] = 0.f;
        lo[r] = 0;
    }
}

}  // namespace

extern "C" int abr_rpn_pyramid_max_k(void);   // rpn_pyramid.hip

extern "C" int abr_retina_max_candidates(void) { return ICAP; }

extern "C" int abr_retina_detect(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host,
                                 const float* const* anchors_host, const int* nloc_host, int L, int N, int A, int C, const int32_t* img_hw,
                                 float score_thresh, int pre_nms_top_n, float nms_thresh, int detections_per_img, float wx, float wy, float ww,
                                 float wh, float min_size, int cap, float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* n_out,
                                 void* stream) {
    ABR_REQUIRE(L >= 1 && L <= MAXL, "retina_detect: L = %d levels, need 1 .. %d", L, MAXL);
    ABR_REQUIRE(N >= 0 && A >= 1 && C >= 1 && pre_nms_top_n >= 1, "retina_detect: bad N, A, C or pre_nms_top_n");
    ABR_REQUIRE(C <= (int)LABEL_MASK - 1 && (long long)A * C <= 0x7FFFFFFF, "retina_detect: C = %d classes, at most %d", C, (int)LABEL_MASK - 1);
    ABR_REQUIRE(pre_nms_top_n <= KCAP && KCAP == abr_rpn_pyramid_max_k(), "retina_detect: pre_nms_top_n = %d, the in-LDS sort ranks %d per (image, level)",
                pre_nms_top_n, KCAP);
    ABR_REQUIRE((long long)L * pre_nms_top_n <= ICAP, "retina_detect: L * pre_nms_top_n = %lld candidates per image, the in-LDS sort holds %d",
                (long long)L * pre_nms_top_n, ICAP);
    ABR_REQUIRE(cap == L * pre_nms_top_n, "retina_detect: cap = %d, need L * pre_nms_top_n = %d", cap, L * pre_nms_top_n);
    ABR_REQUIRE(cls_host && ldc_host && reg_host && ldr_host && anchors_host && nloc_host, "retina_detect: null level table");
    const int K = pre_nms_top_n, AC = A * C;
    RetLevels lv;
    long long off = 0;
    for (int l = 0; l < MAXL; l++) {
        const int s = l < L ? l : 0;     // unused entries repeat level 0
        ABR_REQUIRE(nloc_host[s] >= 1 && ldc_host[s] >= AC && ldr_host[s] >= 4 * A, "retina_detect: level %d: bad nloc / ldc / ldr", s);
        const long long n = (long long)nloc_host[s] * AC;
        ABR_REQUIRE(n <= 0x7FFFFFFF && (long long)std::max(N, 1) * nloc_host[s] * std::max(ldc_host[s], ldr_host[s]) <= 0x7FFFFFFF,
                    "retina_detect: level %d does not fit int32", s);
        ABR_REQUIRE(l >= L || N == 0 || (cls_host[l] && reg_host[l] && anchors_host[l]), "retina_detect: level %d: null pointer", l);
        ABR_REQUIRE((reinterpret_cast<uintptr_t>(anchors_host[s]) & 15) == 0, "retina_detect: level %d: anchors must be 16-byte aligned", s);
        lv.cls[l] = cls_host[s];
        lv.reg[l] = reg_host[s];
        lv.anchors[l] = anchors_host[s];
        lv.nloc[l] = nloc_host[s];
        lv.ldc[l] = ldc_host[s];
        lv.ldr[l] = ldr_host[s];
        lv.n[l] = n;
        lv.k[l] = (int)std::min<long long>(K, n);
        lv.per[l] = (int)((((n + G - 1) / G) + KT - 1) / KT * KT);
        lv.off[l] = off;
        if (l < L) off += (long long)N * n;
    }
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(img_hw && out_boxes && out_scores && out_labels && n_out, "retina_detect: null pointer");
    ABR_REQUIRE((reinterpret_cast<uintptr_t>(out_boxes) & 15) == 0, "retina_detect: out_boxes must be 16-byte aligned");
    ABR_REQUIRE((long long)N * L <= 65535, "retina_detect: N * L = %lld segments, at most 65535", (long long)N * L);
    const size_t S = (size_t)N * L;
    hipStream_t st = abr::as_stream(stream);
    const size_t head = S * HB * 4 + S * sizeof(RetCnt);
    const size_t rows = S * K;
    const size_t bytes = head + S * KCAP * 8 + rows * 16 + rows * 4 + rows * 4 + ((S * 4 + 15) & ~(size_t)15) + (size_t)off * 8 + 16;
    char* b = static_cast<char*>(abr::scratch(abr::SCRATCH_RETINA, st, bytes));
    ABR_REQUIRE(b, "retina_detect: scratch allocation failed");
    int* hist = reinterpret_cast<int*>(b);                                   b += S * HB * 4;
    RetCnt* cnt = reinterpret_cast<RetCnt*>(b);                              b += S * sizeof(RetCnt);
    unsigned long long* surv = reinterpret_cast<unsigned long long*>(b);     b += S * KCAP * 8;
    float* seg_boxes = reinterpret_cast<float*>(b);                          b += rows * 16;
    float* seg_scores = reinterpret_cast<float*>(b);                         b += rows * 4;
    int32_t* seg_labels = reinterpret_cast<int32_t*>(b);                     b += rows * 4;
    int32_t* seg_counts = reinterpret_cast<int32_t*>(b);                     b += (S * 4 + 15) & ~(size_t)15;
    unsigned long long* binl = reinterpret_cast<unsigned long long*>(b);
    int p2 = 2;
    while (p2 < L * K) p2 <<= 1;
    const size_t lds = (size_t)p2 * 8 + HB * 4 + (TT / 64) * 4 + 16 + (size_t)p2;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ret_image_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (hipMemsetAsync(hist, 0, head, st) != hipSuccess) return ABR_E_LAUNCH;
    ret_hist_kernel<<<dim3(G, (unsigned)S), KT, 0, st>>>(lv, L, AC, score_thresh, hist);
    ret_partition_kernel<<<dim3(G, (unsigned)S), KT, 0, st>>>(lv, L, AC, score_thresh, hist, surv, binl, cnt);
    ret_select_decode_kernel<<<(unsigned)S, TT, 0, st>>>(lv, L, A, C, K, surv, binl, cnt, img_hw, wx, wy, ww, wh, min_size, seg_boxes, seg_scores,
                                                         seg_labels, seg_counts);
    ret_image_kernel<<<(unsigned)N, TT, lds, st>>>(L, K, p2, nms_thresh, detections_per_img, cap, seg_boxes, seg_scores, seg_labels, seg_counts,
                                                   out_boxes, out_scores, out_labels, n_out);
    ABR_CHECK_LAUNCH("retina_detect");
    return ABR_OK;
}
