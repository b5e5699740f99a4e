// RPN proposal ranking: sigmoid + sorted top-k per image.
//
// Reference: maskrcnn_benchmark/modeling/rpn/inference.py:87-96
//     objectness = permute_and_flatten(objectness, N, A, 1, H, W).view(N, -1).sigmoid()
//     objectness, topk_idx = objectness.topk(pre_nms_top_n, dim=1, sorted=True)
// (ATen: permute copy, sigmoid, radix-select + segmented sort = ~8 kernels).  Here the objectness logits are read in place
// from the fused NHWC head output (anchor j = row j/A, column j%A: already the flattened order):
//   1. (chip-wide kernel) sigmoid keys once into a scratch + 12-bit histogram;
//   2-5. partition, exact selection of the k-th key, chunk sorts and a merge by rank (below, before topk_partition_kernel);
// the result orders by descending score, equal scores by ascending index, and the first k are written out as fp32 scores + int64 indices.
// Scores are non-negative floats, so their bit patterns order like the values.
#include <algorithm>

#include "rank_select.h"

namespace {

using abr::find_bin_from_top;

constexpr int TT = 1024;
constexpr int CAP = 16384;  // LDS sort capacity (64-bit words)

// raw = 0: abr::sigmoid_key of the logit.  raw = 1 (abr_sort_scores_desc: the score sort of _C.nms): abr::order_key, the order of x itself
__device__ __forceinline__ unsigned score_bits(const float* __restrict__ base, int j, int A, int ld, int raw) {
    const float x = base[(size_t)(j / A) * ld + (j % A)];
    return raw ? abr::order_key(x) : abr::sigmoid_key(x);
}

// Phase 1, chip-wide (grid = G slices x N images): the sigmoid key of every anchor, once, into a scratch + a histogram of the keys' top 12 bits
// (LDS per workgroup, non-empty bins flushed with global atomics).  One workgroup per image used to make FIVE passes over its 143 640 logits with an
// expf each (175 of the kernel's 290 us on one CU), and the step waits for about 60 % of this kernel's time (ABR_TOPK_TWICE probe, MEASUREMENTS.md).
constexpr int KT = 256;      // threads of the key kernel
constexpr int HB = 4096;     // bins of a 12-bit level

__global__ __launch_bounds__(KT) void topk_keys_kernel(const float* __restrict__ logits, int64_t img_stride, int n, int A, int ld, int per,
                                                       unsigned* __restrict__ keys, int* __restrict__ hist, int raw) {
    __shared__ int lh[HB];
    const int img = blockIdx.y;
    for (int i = threadIdx.x; i < HB; i += KT) lh[i] = 0;
    __syncthreads();
    const float* base = logits + (size_t)img * img_stride;
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = score_bits(base, j, A, ld, raw);
        keys[(size_t)img * n + j] = key;
        atomicAdd(&lh[key >> 20], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HB; i += KT)
        if (lh[i]) atomicAdd(&hist[img * HB + i], lh[i]);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Round 4: phases 2-5 spread over the chip (round 3's one-workgroup-per-image form spent 130 of its 178 us in a 16384-word bitonic sort on ONE CU
// per image, and the step waits for ~60 % of this chain).
//   2. partition (chip-wide, one workgroup per key slice): the level-1 bin b1 that holds the k-th key is read off the histogram by every workgroup;
//      keys above the bin are survivors for certain, keys inside it are CANDIDATES; both are appended to per-image arrays as 64-bit
//      (key << 32 | ~index) words (positions reserved per workgroup: two global atomics per slice);
//   3. select (one workgroup per image): two more radix levels over the CANDIDATES only (a few thousand words, not the 143 640 keys) give the exact
//      k-th key; candidates >= it join the survivors, ties included -- unless the ties would overflow the sort capacity: then three more levels
//      over ~index pick exactly the lowest-index ties that are wanted, so k <= filled <= CAP always and the result never depends on which
//      workgroup won an atomic; the tail of the last 1024-word chunk is zero-filled; cleans the histogram;
//   4. chunk sort (one 256-thread workgroup per 1024 survivors): bitonic sort in LDS, descending;
//   5. merge by rank (one workgroup per chunk): all sorted chunks of the image in LDS; an element's final position = its position in its own chunk
//      + the number of larger elements in every other chunk (binary searches); words are unique (they carry the index), so positions are too;
//      the first k positions are written out as fp32 scores + int64 indices.
// Outputs were identical to the one-workgroup form's (descending score, equal scores by ascending index).
struct TopkCnt { int surv, cand, filled, pad; };
constexpr int CH = 1024;      // words per sorted chunk
constexpr int MAXCH = CAP / CH;

__global__ __launch_bounds__(KT) void topk_partition_kernel(const unsigned* __restrict__ keys_all, const int* __restrict__ hist_all, int n, int k, int per,
                                                            unsigned long long* __restrict__ surv_all, unsigned long long* __restrict__ cand_all,
                                                            TopkCnt* __restrict__ cnt_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* st_s = reinterpret_cast<unsigned long long*>(smem);   // [per] staged survivors of this slice
    unsigned long long* st_c = st_s + per;                                     // [per] staged candidates
    __shared__ int h[HB];
    __shared__ int s_bin, s_krem, n_s, n_c, base_s, base_c;
    const int img = blockIdx.y;
    const unsigned* keys = keys_all + (size_t)img * n;
    const int* hist = hist_all + img * HB;
    for (int i = threadIdx.x; i < HB; i += KT) h[i] = hist[i];
    if (threadIdx.x == 0) { s_krem = k; s_bin = 0; n_s = 0; n_c = 0; }
    __syncthreads();
    int b1 = -1;                       // k == n: every key survives
    if (k < n) {
        find_bin_from_top(h, HB, &s_bin, &s_krem);
        __syncthreads();
        b1 = s_bin;
    }
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = keys[j];
        const int bin = (int)(key >> 20);
        const unsigned long long w = abr::rank_word(key, (unsigned)j);
        if (bin > b1) st_s[atomicAdd(&n_s, 1)] = w;
        else if (bin == b1) st_c[atomicAdd(&n_c, 1)] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        base_s = n_s ? atomicAdd(&cnt_all[img].surv, n_s) : 0;
        base_c = n_c ? atomicAdd(&cnt_all[img].cand, n_c) : 0;
    }
    __syncthreads();
    unsigned long long* surv = surv_all + (size_t)img * CAP;
    unsigned long long* cand = cand_all + (size_t)img * n;
    for (int i = threadIdx.x; i < n_s; i += KT)
        if (base_s + i < CAP) surv[base_s + i] = st_s[i];
    for (int i = threadIdx.x; i < n_c; i += KT) cand[base_c + i] = st_c[i];
}

__global__ __launch_bounds__(TT) void topk_select_kernel(int* __restrict__ hist_all, int n, int k, unsigned long long* __restrict__ surv_all,
                                                         const unsigned long long* __restrict__ cand_all, TopkCnt* __restrict__ cnt_all) {
    __shared__ int h[HB];
    __shared__ int s_bin, s_krem, s_fill;
    const int img = blockIdx.x;
    int* hist = hist_all + img * HB;
    for (int i = threadIdx.x; i < HB; i += TT) { h[i] = hist[i]; hist[i] = 0; }   // the histogram is clean again for the next call
    if (threadIdx.x == 0) { s_krem = k; s_fill = 0; s_bin = 0; }
    __syncthreads();
    const int nsurv = min(cnt_all[img].surv, CAP), ncand = cnt_all[img].cand;
    unsigned long long* surv = surv_all + (size_t)img * CAP;
    const unsigned long long* cand = cand_all + (size_t)img * n;
    if (k < n) {
        find_bin_from_top(h, HB, &s_bin, &s_krem);       // b1 again (the partition's choice), s_krem = how many of the candidates are wanted
        __syncthreads();
        const unsigned b1 = (unsigned)s_bin;
        for (int i = threadIdx.x; i < HB; i += TT) h[i] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < ncand; j += TT) atomicAdd(&h[(unsigned)(cand[j] >> 40) & (HB - 1)], 1);   // key bits 19..8
        __syncthreads();
        find_bin_from_top(h, HB, &s_bin, &s_krem);
        __syncthreads();
        const unsigned p24 = (b1 << 12) | (unsigned)s_bin;
        for (int i = threadIdx.x; i < 256; i += TT) h[i] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < ncand; j += TT) {
            const unsigned key = (unsigned)(cand[j] >> 32);
            if ((key >> 8) == p24) atomicAdd(&h[key & 255], 1);
        }
        __syncthreads();
        find_bin_from_top(h, 256, &s_bin, &s_krem);
        __syncthreads();
        const unsigned thr = (p24 << 8) | (unsigned)s_bin;
        // s_krem of the h[s_bin] words whose key IS thr are wanted; the survivors and the candidates above thr make up the other k - s_krem
        const int want_eq = s_krem, n_eq = h[s_bin];
        __syncthreads();
        if (k - want_eq + n_eq <= CAP) {
            for (int j = threadIdx.x; j < ncand; j += TT) {   // every tie of the k-th key joins: they fit, and the merge emits the first k
                const unsigned long long w = cand[j];
                if ((unsigned)(w >> 32) >= thr) {
                    const int pos = nsurv + atomicAdd(&s_fill, 1);
                    if (pos < CAP) surv[pos] = w;
                }
            }
        } else {
            // More ties of the k-th key than the sort holds (zero-padded batches: thousands of identical logits).  Which of them join must not be
            // left to the order in which the atomics above and in the partition were won: the selection goes on over the words' low halves
            // (~index: 12 + 12 + 8 bits, as over the keys) among the words whose key is thr, down to the k-th WORD, and exactly the words at or
            // above it join -- the lowest indices of the tie group, nsurv + joined == k.
            unsigned long long pre = 0ull;                    // the k-th word's low bits found so far
            for (int lv = 0; lv < 3; lv++) {
                const int sh = lv == 0 ? 20 : lv == 1 ? 8 : 0, bits = lv == 2 ? 8 : 12, nb = 1 << bits;
                for (int i = threadIdx.x; i < nb; i += TT) h[i] = 0;
                __syncthreads();
                for (int j = threadIdx.x; j < ncand; j += TT) {
                    const unsigned long long w = cand[j], low = w & 0xFFFFFFFFull;
                    if ((unsigned)(w >> 32) == thr && (low >> (sh + bits)) == pre) atomicAdd(&h[(unsigned)(low >> sh) & (nb - 1)], 1);
                }
                __syncthreads();
                find_bin_from_top(h, nb, &s_bin, &s_krem);
                __syncthreads();
                pre = (pre << bits) | (unsigned)s_bin;
            }
            const unsigned long long thrw = ((unsigned long long)thr << 32) | pre;
            for (int j = threadIdx.x; j < ncand; j += TT) {
                const unsigned long long w = cand[j];
                if (w >= thrw) {
                    const int pos = nsurv + atomicAdd(&s_fill, 1);
                    if (pos < CAP) surv[pos] = w;
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();   // (k == n: nothing above separates the reads of the counters from their reset below)
    const int filled = min(nsurv + s_fill, CAP);
    for (int j = filled + threadIdx.x; j < (filled + CH - 1) / CH * CH; j += TT) surv[j] = 0ull;   // padding sorts last
    if (threadIdx.x == 0) { cnt_all[img].filled = filled; cnt_all[img].surv = 0; cnt_all[img].cand = 0; }
}

__global__ __launch_bounds__(256) void topk_chunk_sort_kernel(unsigned long long* __restrict__ surv_all, const TopkCnt* __restrict__ cnt_all) {
    __shared__ unsigned long long buf[CH];
    const int img = blockIdx.y, c = blockIdx.x;
    if (c * CH >= cnt_all[img].filled) return;
    unsigned long long* a = surv_all + (size_t)img * CAP + (size_t)c * CH;
    for (int i = threadIdx.x; i < CH; i += 256) buf[i] = a[i];
    __syncthreads();
    abr::bitonic_desc<256>(buf, CH);
    for (int i = threadIdx.x; i < CH; i += 256) a[i] = buf[i];
}

__global__ __launch_bounds__(TT) void topk_merge_emit_kernel(const unsigned long long* __restrict__ surv_all, const TopkCnt* __restrict__ cnt_all, int k,
                                                             float* __restrict__ scores, int64_t* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* buf = reinterpret_cast<unsigned long long*>(smem);   // [nch][CH]: every sorted chunk of the image
    const int img = blockIdx.y, c = blockIdx.x;
    const int filled = cnt_all[img].filled;
    if (c * CH >= filled) return;              // (filled >= k: the select phase joins every wanted word, and never more than CAP)
    const int nch = (filled + CH - 1) / CH;
    const uint4* src = reinterpret_cast<const uint4*>(surv_all + (size_t)img * CAP);
    uint4* dst = reinterpret_cast<uint4*>(buf);
    for (int i = threadIdx.x; i < nch * (CH / 2); i += TT) dst[i] = src[i];
    __syncthreads();
    const int t = threadIdx.x;
    const unsigned long long x = buf[c * CH + t];
    if (x == 0ull) return;                     // padding
    int rank = t;
    for (int o = 0; o < nch; o++) {
        if (o == c) continue;
        const unsigned long long* a = buf + o * CH;   // descending: count the elements larger than x
        int lo = 0, hi = CH;
#pragma unroll
        for (int it = 0; it < 11; it++) {          // 1025 possible answers (0 .. CH): 11 halvings; once lo == hi the steps are no-ops
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a[mid] > x) lo = mid + 1; else hi = mid;
            }
        }
        rank += lo;
    }
    if (rank < k) {
        if (scores) scores[(size_t)img * k + rank] = __uint_as_float(abr::rank_word_key(x));
        idx[(size_t)img * k + rank] = (int64_t)abr::rank_word_index(x);
    }
}

}  // namespace

static int topk_run(const float* logits, int64_t img_stride, int N, int n, int A, int ld, int k, float* scores, int64_t* idx, int raw, void* stream);

extern "C" int abr_topk_sigmoid(const float* logits, int64_t img_stride, int N, int n, int A, int ld, int k, float* scores,
                                int64_t* idx, void* stream) {
    ABR_REQUIRE(N >= 0 && n > 0 && A >= 1 && ld >= A && k >= 0 && k <= n, "topk_sigmoid: bad args");
    ABR_REQUIRE(k <= CAP - 1024, "topk_sigmoid: k too large for the in-LDS sort (max 15360)");
    if (N == 0 || k == 0) return ABR_OK;
    ABR_REQUIRE(logits && scores && idx, "topk_sigmoid: null pointer");
    return topk_run(logits, img_stride, N, n, A, ld, k, scores, idx, 0, stream);
}

extern "C" int64_t abr_sort_scores_max_n(void) { return CAP - 1024; }

extern "C" int abr_sort_scores_desc(const float* scores, int n, int64_t* order, void* stream) {
    ABR_REQUIRE(n >= 0 && n <= CAP - 1024, "sort_scores_desc: at most 15360 scores");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(scores && order, "sort_scores_desc: null pointer");
    return topk_run(scores, n, 1, n, 1, 1, n, nullptr, order, 1, stream);
}

static int topk_run(const float* logits, int64_t img_stride, int N, int n, int A, int ld, int k, float* scores, int64_t* idx, int raw, void* stream) {
    const int G = 64;
    const int per = ((n + G - 1) / G + KT - 1) / KT * KT;
    const size_t lds_sort = (size_t)CAP * 8, lds_part = (size_t)per * 16;
    // the partition kernel keeps its slice's keys in LDS beside 16 KB of histogram: beyond 64 KB (n > ~196 k keys per image; the C4 geometries of
    // this path stay below 63 k) it cannot be launched -- say so instead of returning a launch error
    ABR_REQUIRE(lds_part + 16384 <= 65536, "topk_sigmoid: %d keys per image exceed the partition kernel's LDS (at most 196608)", n);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_merge_emit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sort);
        // (the largest admitted slice stages 48 KB beside the partition kernel's 16 KB histogram and its few scalars: a little over 64 KB in all)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_partition_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 49152);
        attr = true;
    }
    // scratch per stream (launches on a stream are ordered), all of it at offsets that depend on CAPACITIES only:
    //   [level-1 histograms: cap_imgs x 4096][counters: cap_imgs][survivors: cap_imgs x CAP words][keys: cap_keys][candidates: cap_keys words]
    // The histogram and counter regions are zero on entry (allocation zero-fills them, the select phase cleans what it used); their position does not
    // depend on n or N, so a later call with a smaller feature map / another batch size never finds stale key bits where it expects zeros.
    // Grow-only: keyed on capacity, not on N ==.  The capacities (images, keys) are the entry's two words; the bytes they ask for grow with
    // either, so a request within both fits and touches nothing.
    hipStream_t st = abr::as_stream(stream);
    unsigned* keys;
    int* hist;
    TopkCnt* cnt;
    unsigned long long *surv, *cand;
    const bool have = abr::scratch_pool().locked(abr::SCRATCH_TOPK, st, [&](abr::ScratchPool::Ref w) {
        const size_t imgs = std::max<size_t>(std::max<size_t>((size_t)N, w.words[0]), 8);
        const size_t nkeys = std::max<size_t>((size_t)N * n, w.words[1]);
        const size_t head = imgs * HB * 4 + imgs * sizeof(TopkCnt);
        char* b = static_cast<char*>(w.ensure(head + imgs * CAP * 8 + nkeys * 4 + nkeys * 8 + 16, head));
        if (!b) return false;
        w.words[0] = imgs;
        w.words[1] = nkeys;
        hist = reinterpret_cast<int*>(b);                          b += imgs * HB * 4;
        cnt = reinterpret_cast<TopkCnt*>(b);                       b += imgs * sizeof(TopkCnt);
        surv = reinterpret_cast<unsigned long long*>(b);           b += imgs * CAP * 8;
        cand = reinterpret_cast<unsigned long long*>(b);           b += nkeys * 8;
        keys = reinterpret_cast<unsigned*>(b);
        return true;
    });
    ABR_REQUIRE(have, "topk_sigmoid: scratch allocation failed");
    const unsigned slices = (unsigned)((n + per - 1) / per);
    topk_keys_kernel<<<dim3(slices, (unsigned)N), KT, 0, st>>>(logits, img_stride, n, A, ld, per, keys, hist, raw);
    topk_partition_kernel<<<dim3(slices, (unsigned)N), KT, lds_part, st>>>(keys, hist, n, k, per, surv, cand, cnt);
    topk_select_kernel<<<N, TT, 0, st>>>(hist, n, k, surv, cand, cnt);
    topk_chunk_sort_kernel<<<dim3(MAXCH, (unsigned)N), 256, 0, st>>>(surv, cnt);
    topk_merge_emit_kernel<<<dim3(MAXCH, (unsigned)N), TT, lds_sort, st>>>(surv, cnt, k, scores, idx);
    ABR_CHECK_LAUNCH("topk_sigmoid");
    return ABR_OK;
}
