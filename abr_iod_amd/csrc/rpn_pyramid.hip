// RPN proposal selection over a feature pyramid: every (image, level) SEGMENT goes through each stage together, nothing is read back.
//
// Reference: maskrcnn_benchmark/modeling/rpn/inference.py:76-118 per level (permute, sigmoid, topk, two gathers, decode; per image a clip, a
// nonzero, an NMS with a host loop) and :149-176 across the levels (cat, topk, mask scatter, boolean index per image): for five levels and two
// images well over a hundred launches and a dozen host synchronisations.  Here, with S = N * L segments:
//
//   abr_rpn_pyramid_topk    1 memset + 3 launches, whatever N and L are
//     1. keys (grid: slices x S): the sigmoid key of every anchor of every level, once, into scratch + a histogram of the keys' top 12 bits per
//        segment (LDS per workgroup, flushed with integer atomics).  The key is abr_topk_sigmoid's: abr::sigmoid_key (rank_select.h).
//     2. partition (grid: slices x S): the bin b1 holding the k-th key is read off the histogram by every workgroup; words (abr::rank_word: key << 32 | ~index)
//        of keys above the bin are SURVIVORS (fewer than k of them), words inside it CANDIDATES; both are appended per segment (a counting pass,
//        one reservation per workgroup with two global integer atomics, a writing pass: no staging in LDS, so no limit on the slice).
//     3. select + sort + emit (one 1024-thread workgroup per segment): the words are unique, so the (k - #survivors)-th largest candidate WORD
//        is found exactly by five more radix levels (key bits 19..8, 7..0, then ~index 31..20, 19..8, 7..0) over the candidates only; the
//        candidates at or above it join the survivors -- exactly k words, whichever workgroup won which atomic -- and a bitonic sort in LDS
//        orders them: descending score, equal scores by ascending index (abr_topk_sigmoid's order).
//     LDS per workgroup: 16 KB histogram (all three kernels) + 16 KB sort buffer (kernel 3: 2048 64-bit words) = 32 KB of a CU's 160 KB.
//     Hence k_l <= 2048 (abr_rpn_pyramid_max_k): FPN configurations rank 1000 to 2000 per level.  Over the cap the call is an error.
//     Scratch (per stream, from the pool): [histograms S x 4096][counters S][survivors S x 2048 words][candidates: a word per key][keys].
//     Histograms and counters are zeroed by the call itself, everything else is written before it is read: no call depends on what an earlier
//     one (a larger pyramid, another batch size) left behind.
//   abr_rpn_pyramid_decode  1 launch (one workgroup per segment): BoxCoder.decode + clip_to_image through the functions decode_clip_kernel
//     (rpn.hip) calls (abr::box_decode, box_clip: box_math.h), remove_small_boxes, and a stable compaction (wave ballots + a prefix over the 16 waves) so that survivors keep rank order.
//   abr_nms_sorted_batched  (nms.hip, unchanged) with the S segments as its "images"
//   abr_rpn_pyramid_select  3 launches: candidate words (order-preserving score key << 32 | ~position), the exact k-th largest word by a
//     six-level radix selection (one workgroup per image, or one for the batch in mode 1), emission (one workgroup per image: mode 0 sorts the
//     chosen words in LDS -- at most 4096 of them, 32 KB; mode 1 compacts them in candidate order).  Words are unique, the threshold is exact:
//     no result depends on the order in which atomics were won.
#include <algorithm>

#include "box_math.h"
#include "rank_select.h"

namespace {

using abr::find_bin_from_top;
using abr::kth_word;

constexpr int MAXL = ABR_MAX_PYRAMID_LEVELS;
constexpr int KT = 256;       // threads of the chip-wide kernels
constexpr int TT = 1024;      // threads of the per-segment kernels
constexpr int HB = 4096;      // bins of a 12-bit level
constexpr int KCAP = 2048;    // most keys ranked per segment (the in-LDS sort)
constexpr int SELCAP = 4096;  // most proposals emitted per image in mode 0 (the in-LDS sort)
constexpr int G = 64;         // key slices per segment

struct PyrLevels {            // by value in the kernel arguments: no device-side table
    const float* y[MAXL];         // [N, nloc, ld] fused head output of the level
    const float* anchors[MAXL];   // [nloc * A, 4] (decode only)
    int n[MAXL], A[MAXL], ld[MAXL], k[MAXL], per[MAXL];
    long long key0[MAXL];         // offset of the level's keys [N, n] in the key / candidate scratch
};
struct PyrCnt { int surv, cand; };
struct SelThr { unsigned long long word; int want, total; };

// ---------------------------------------------------------------------------------------------------------------------------- ranking
__global__ __launch_bounds__(KT) void pyr_keys_kernel(PyrLevels lv, int L, unsigned* __restrict__ keys, int* __restrict__ hist) {
    __shared__ int lh[HB];
    const int seg = blockIdx.y, img = seg / L, l = seg % L;
    const int n = lv.n[l], A = lv.A[l], ld = lv.ld[l], per = lv.per[l];
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    if (j0 >= n) return;
    for (int i = threadIdx.x; i < HB; i += KT) lh[i] = 0;
    __syncthreads();
    const float* base = lv.y[l] + (size_t)img * (n / A) * ld;
    unsigned* kout = keys + lv.key0[l] + (size_t)img * n;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const float x = base[(size_t)(j / A) * ld + (j % A)];
        const unsigned key = abr::sigmoid_key(x);
        kout[j] = key;
        atomicAdd(&lh[key >> 20], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HB; i += KT)
        if (lh[i]) atomicAdd(&hist[(size_t)seg * HB + i], lh[i]);
}

__global__ __launch_bounds__(KT) void pyr_partition_kernel(PyrLevels lv, int L, const unsigned* __restrict__ keys_all, const int* __restrict__ hist,
                                                           unsigned long long* __restrict__ surv_all, unsigned long long* __restrict__ cand_all,
                                                           PyrCnt* __restrict__ cnt_all) {
    __shared__ int h[HB];
    __shared__ int s_bin, s_krem, n_s, n_c, base_s, base_c;
    const int seg = blockIdx.y, img = seg / L, l = seg % L;
    const int n = lv.n[l], k = lv.k[l], per = lv.per[l];
    const int j0 = blockIdx.x * per, j1 = min(j0 + per, n);
    if (j0 >= n) return;
    const unsigned* keys = keys_all + lv.key0[l] + (size_t)img * n;
    if (threadIdx.x == 0) { s_krem = k; s_bin = 0; n_s = 0; n_c = 0; }
    int b1 = -1;                       // k == n: every key survives
    if (k < n) {
        for (int i = threadIdx.x; i < HB; i += KT) h[i] = hist[(size_t)seg * HB + i];
        __syncthreads();
        find_bin_from_top(h, HB, &s_bin, &s_krem);
        __syncthreads();
        b1 = s_bin;
    } else {
        __syncthreads();
    }
    int my_s = 0, my_c = 0;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const int bin = (int)(keys[j] >> 20);
        my_s += bin > b1;
        my_c += bin == b1;
    }
    if (my_s) atomicAdd(&n_s, my_s);
    if (my_c) atomicAdd(&n_c, my_c);
    __syncthreads();
    if (threadIdx.x == 0) {
        base_s = n_s ? atomicAdd(&cnt_all[seg].surv, n_s) : 0;
        base_c = n_c ? atomicAdd(&cnt_all[seg].cand, n_c) : 0;
        n_s = 0;
        n_c = 0;
    }
    __syncthreads();
    unsigned long long* surv = surv_all + (size_t)seg * KCAP;
    unsigned long long* cand = cand_all + lv.key0[l] + (size_t)img * n;
    for (int j = j0 + threadIdx.x; j < j1; j += KT) {
        const unsigned key = keys[j];
        const int bin = (int)(key >> 20);
        const unsigned long long w = abr::rank_word(key, (unsigned)j);
        if (bin > b1) {
            const int pos = base_s + atomicAdd(&n_s, 1);
            if (pos < KCAP) surv[pos] = w;
        } else if (bin == b1) {
            cand[base_c + atomicAdd(&n_c, 1)] = w;     // (at most n candidates: the region holds n words)
        }
    }
}

__global__ __launch_bounds__(TT) void pyr_select_sort_kernel(PyrLevels lv, int L, int k_max, const unsigned long long* __restrict__ surv_all,
                                                             const unsigned long long* __restrict__ cand_all, const PyrCnt* __restrict__ cnt_all,
                                                             float* __restrict__ scores, int64_t* __restrict__ idx) {
    __shared__ int h[HB];
    __shared__ unsigned long long buf[KCAP];
    __shared__ int s_bin, s_krem, s_fill;
    const int seg = blockIdx.x, img = seg / L, l = seg % L;
    const int n = lv.n[l], k = lv.k[l];
    const int nsurv = min(cnt_all[seg].surv, k), ncand = min(cnt_all[seg].cand, n);
    const unsigned long long* surv = surv_all + (size_t)seg * KCAP;
    const unsigned long long* cand = cand_all + lv.key0[l] + (size_t)img * n;
    int p2 = 2;
    while (p2 < k) p2 <<= 1;
    for (int i = threadIdx.x; i < p2; i += TT) buf[i] = i < nsurv ? surv[i] : 0ull;    // padding sorts last
    if (threadIdx.x == 0) s_fill = 0;
    __syncthreads();
    const int want = k - nsurv;
    if (want > 0 && ncand > 0) {
        const unsigned long long thrw = kth_word(cand, ncand, min(want, ncand), 1, cand[0] >> 52, h, &s_bin, &s_krem);
        for (int j = threadIdx.x; j < ncand; j += TT) {
            const unsigned long long w = cand[j];
            if (w >= thrw) {
                const int pos = nsurv + atomicAdd(&s_fill, 1);
                if (pos < k) buf[pos] = w;
            }
        }
        __syncthreads();
    }
    abr::bitonic_desc<TT>(buf, p2);
    float* so = scores + (size_t)seg * k_max;
    int64_t* io = idx + (size_t)seg * k_max;
    for (int r = threadIdx.x; r < k_max; r += TT) {
        const unsigned long long x = r < k ? buf[r] : 0ull;
        so[r] = r < k ? __uint_as_float(abr::rank_word_key(x)) : 0.f;
        io[r] = r < k ? (int64_t)abr::rank_word_index(x) : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- decode
#pragma clang fp contract(off)
__global__ __launch_bounds__(TT) void pyr_decode_kernel(PyrLevels lv, int L, int k_max, const int64_t* __restrict__ idx, const float* __restrict__ scores_in,
                                                        const int32_t* __restrict__ img_hw, float wx, float wy, float ww, float wh, float min_size,
                                                        float* __restrict__ props, float* __restrict__ scores_out, int32_t* __restrict__ counts) {
    __shared__ int s_wave[TT / 64];
    __shared__ int s_base;
    const int seg = blockIdx.x, i = seg / L, l = seg % L;
    const int k = lv.k[l], A = lv.A[l], ld = lv.ld[l], nloc = lv.n[l] / A;
    const float* reg = lv.y[l];
    const float* anchors = lv.anchors[l];
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    float4* po = reinterpret_cast<float4*>(props) + (size_t)seg * k_max;
    float* so = scores_out + (size_t)seg * k_max;
    for (int c0 = 0; c0 < k; c0 += TT) {
        const int t = c0 + threadIdx.x;
        bool keep = false;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        if (t < k) {
            const int64_t a = idx[(size_t)seg * k_max + t];
            sc = scores_in[(size_t)seg * k_max + t];
            const float* d = reg + ((size_t)i * nloc + a / A) * ld + A + 4 * (a % A);
            o = abr::box_decode(reinterpret_cast<const float4*>(anchors)[a], d, wx, wy, ww, wh);
            o = abr::box_clip(o, (float)(img_hw[2 * i + 1] - 1), (float)(img_hw[2 * i] - 1));
            // boxlist_ops.py:34-48 remove_small_boxes; min_size <= 0 keeps every row, as the single-level path does
            keep = min_size <= 0.f || ((o.z - o.x + 1 >= min_size) && (o.w - o.y + 1 >= min_size));
        }
        const int pos = abr::compact_pos<TT>(keep, s_wave, &s_base);
        if (keep) {
            po[pos] = o;
            so[pos] = sc;
        }
    }
    const int count = s_base;
    if (threadIdx.x == 0) counts[seg] = count;
    for (int r = count + threadIdx.x; r < k_max; r += TT) {
        po[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        so[r] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- selection
// candidate position g = (image * L + level) * post + rank -> its word, 0 where the level kept fewer than rank + 1 boxes
__global__ void sel_words_kernel(const float* __restrict__ scores, const int32_t* __restrict__ keep, const int32_t* __restrict__ n_keep, int total, int k_max,
                                 int post, unsigned long long* __restrict__ words) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int seg = g / post, r = g % post;
    unsigned long long w = 0ull;
    if (r < min(n_keep[seg], post)) {
        const int row = keep[(size_t)seg * post + r];
        w = abr::rank_word(abr::order_key(scores[(size_t)seg * k_max + row]), (unsigned)g);
    }
    words[g] = w;
}

// group = image (mode 0) or the whole batch (mode 1): want = min(fpn_post_n, #candidates) and the want-th largest word
__global__ __launch_bounds__(TT) void sel_threshold_kernel(const unsigned long long* __restrict__ words, int per_group, int fpn_post_n,
                                                           SelThr* __restrict__ thr) {
    __shared__ int h[HB];
    __shared__ int s_bin, s_krem, s_total;
    const unsigned long long* a = words + (size_t)blockIdx.x * per_group;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < per_group; j += TT) mine += a[j] != 0ull;
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    const int total = s_total, want = min(fpn_post_n, total);
    unsigned long long w = ~0ull;
    if (want > 0) w = kth_word(a, per_group, want, 0, 0ull, h, &s_bin, &s_krem);
    if (threadIdx.x == 0) {
        thr[blockIdx.x].word = w;
        thr[blockIdx.x].want = want;
        thr[blockIdx.x].total = total;
    }
}

__global__ __launch_bounds__(TT) void sel_emit_kernel(const unsigned long long* __restrict__ words, const SelThr* __restrict__ thr, int mode, int L, int k_max,
                                                      int post, int cap, const float* __restrict__ props, const float* __restrict__ scores,
                                                      const int32_t* __restrict__ keep, float* __restrict__ rois, float* __restrict__ out_scores,
                                                      int32_t* __restrict__ src, int32_t* __restrict__ n_out) {
    __shared__ unsigned long long buf[SELCAP];
    __shared__ int s_wave[TT / 64];
    __shared__ int s_base;
    const int i = blockIdx.x, per_img = L * post;
    const SelThr t = thr[mode ? 0 : i];
    const unsigned long long* a = words + (size_t)i * per_img;
    float4* ro = reinterpret_cast<float4*>(rois) + (size_t)i * cap;
    float* so = out_scores + (size_t)i * cap;
    int32_t* po = src + (size_t)i * cap;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    int count;
    if (mode == 0) {
        // the chosen words (exactly t.want of them), sorted: descending score, equal scores by ascending candidate position
        count = t.want;
        int p2 = 2;
        while (p2 < count) p2 <<= 1;
        for (int r = threadIdx.x; r < p2; r += TT) buf[r] = 0ull;
        __syncthreads();
        if (count > 0) {
            for (int j = threadIdx.x; j < per_img; j += TT) {
                const unsigned long long w = a[j];
                if (w != 0ull && w >= t.word) {
                    const int pos = atomicAdd(&s_base, 1);
                    if (pos < SELCAP) buf[pos] = w;
                }
            }
            __syncthreads();
            abr::bitonic_desc<TT>(buf, p2);
            for (int r = threadIdx.x; r < count; r += TT) {
                const int p = (int)abr::rank_word_index(buf[r]) - i * per_img;
                const int seg = i * L + p / post;
                const int row = keep[(size_t)seg * post + p % post];
                ro[r] = reinterpret_cast<const float4*>(props)[(size_t)seg * k_max + row];
                so[r] = scores[(size_t)seg * k_max + row];
                po[r] = p;
            }
        }
    } else {
        // the batch's chosen words that belong to this image, in candidate order (the reference indexes with a mask)
        for (int c0 = 0; c0 < per_img; c0 += TT) {
            const int p = c0 + threadIdx.x;
            const unsigned long long w = p < per_img ? a[p] : 0ull;
            const bool take = t.want > 0 && w != 0ull && w >= t.word;
            const int pos = abr::compact_pos<TT>(take, s_wave, &s_base);
            if (take && pos < cap) {
                const int seg = i * L + p / post;
                const int row = keep[(size_t)seg * post + p % post];
                ro[pos] = reinterpret_cast<const float4*>(props)[(size_t)seg * k_max + row];
                so[pos] = scores[(size_t)seg * k_max + row];
                po[pos] = p;
            }
        }
        count = min(s_base, cap);
    }
    if (threadIdx.x == 0) n_out[i] = count;
    for (int r = count + threadIdx.x; r < cap; r += TT) {
        ro[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        so[r] = 0.f;
        po[r] = -1;
    }
}

// the levels' host tables -> the kernels' by-value argument; checks what every entry checks
int fill_levels(const char* name, PyrLevels& lv, const float* const* y, const int* nloc, const int* A, const int* ld, const float* const* anchors, int L,
                int N, int pre, int k_max, bool decode) {
    ABR_REQUIRE(L >= 1 && L <= MAXL, "%s: L = %d levels, need 1 .. %d", name, L, MAXL);
    ABR_REQUIRE(N >= 0 && pre >= 1, "%s: bad N or pre_nms_top_n", name);
    ABR_REQUIRE(y && nloc && A && ld, "%s: null level table", name);
    long long off = 0;
    int km = 0;
    for (int l = 0; l < MAXL; l++) {
        const int s = l < L ? l : 0;     // unused entries repeat level 0
        ABR_REQUIRE(nloc[s] >= 1 && A[s] >= 1 && ld[s] >= A[s], "%s: level %d: bad nloc / A / ld", name, s);
        ABR_REQUIRE(!decode || ld[s] >= 5 * A[s], "%s: level %d: ld = %d holds no 4A delta columns behind the A logits", name, s, ld[s]);
        const long long n = (long long)nloc[s] * A[s];
        ABR_REQUIRE(n <= 0x7FFFFFFF && (long long)std::max(N, 1) * nloc[s] * ld[s] <= 0x7FFFFFFF, "%s: level %d does not fit int32", name, s);
        lv.y[l] = y[s];
        lv.anchors[l] = anchors ? anchors[s] : nullptr;
        lv.n[l] = (int)n;
        lv.A[l] = A[s];
        lv.ld[l] = ld[s];
        lv.k[l] = (int)std::min<long long>(pre, n);
        lv.per[l] = (int)((((n + G - 1) / G) + KT - 1) / KT * KT);
        lv.key0[l] = off;
        if (l < L) {
            ABR_REQUIRE(N == 0 || (y[l] && (!anchors || anchors[l])), "%s: level %d: null pointer", name, l);
            ABR_REQUIRE(decode || lv.k[l] <= KCAP, "%s: level %d ranks %d keys, the in-LDS sort holds %d", name, l, lv.k[l], KCAP);
            off += (long long)N * n;
            km = std::max(km, lv.k[l]);
        }
    }
    ABR_REQUIRE(off <= 0x7FFFFFFF, "%s: %lld keys do not fit int32", name, off);
    ABR_REQUIRE(k_max == km, "%s: k_max = %d, the levels' largest k is %d", name, k_max, km);
    ABR_REQUIRE((long long)N * L * k_max * 4 <= 0x7FFFFFFF, "%s: N * L * k_max does not fit int32", name);
    return ABR_OK;
}

}  // namespace

extern "C" int abr_rpn_pyramid_max_k(void) { return KCAP; }

extern "C" int abr_rpn_pyramid_topk(const float* const* y_host, const int* nloc_host, const int* A_host, const int* ld_host, int L, int N,
                                    int pre_nms_top_n, int k_max, float* scores, int64_t* idx, void* stream) {
    PyrLevels lv;
    const int rc = fill_levels("rpn_pyramid_topk", lv, y_host, nloc_host, A_host, ld_host, nullptr, L, N, pre_nms_top_n, k_max, false);
    if (rc != ABR_OK) return rc;
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(scores && idx, "rpn_pyramid_topk: null pointer");
    const size_t S = (size_t)N * L;
    size_t nkeys = 0;
    for (int l = 0; l < L; l++) nkeys += (size_t)N * lv.n[l];
    hipStream_t st = abr::as_stream(stream);
    const size_t head = S * HB * 4 + S * sizeof(PyrCnt);
    char* b = static_cast<char*>(abr::scratch(abr::SCRATCH_RPN_PYRAMID, st, head + S * KCAP * 8 + nkeys * 8 + nkeys * 4 + 16));
    ABR_REQUIRE(b, "rpn_pyramid_topk: scratch allocation failed");
    int* hist = reinterpret_cast<int*>(b);                                   b += S * HB * 4;
    PyrCnt* cnt = reinterpret_cast<PyrCnt*>(b);                              b += S * sizeof(PyrCnt);
    unsigned long long* surv = reinterpret_cast<unsigned long long*>(b);     b += S * KCAP * 8;
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(b);     b += nkeys * 8;
    unsigned* keys = reinterpret_cast<unsigned*>(b);
    if (hipMemsetAsync(hist, 0, head, st) != hipSuccess) return ABR_E_LAUNCH;
    pyr_keys_kernel<<<dim3(G, (unsigned)S), KT, 0, st>>>(lv, L, keys, hist);
    pyr_partition_kernel<<<dim3(G, (unsigned)S), KT, 0, st>>>(lv, L, keys, hist, surv, cand, cnt);
    pyr_select_sort_kernel<<<(unsigned)S, TT, 0, st>>>(lv, L, k_max, surv, cand, cnt, scores, idx);
    ABR_CHECK_LAUNCH("rpn_pyramid_topk");
    return ABR_OK;
}

extern "C" int abr_rpn_pyramid_decode(const float* const* y_host, const int* nloc_host, const int* A_host, const int* ld_host,
                                      const float* const* anchors_host, int L, int N, int pre_nms_top_n, int k_max, const int64_t* idx,
                                      const float* scores_in, const int32_t* img_hw, float wx, float wy, float ww, float wh, float min_size,
                                      float* props, float* scores_out, int32_t* counts, void* stream) {
    PyrLevels lv;
    ABR_REQUIRE(anchors_host, "rpn_pyramid_decode: null level table");
    const int rc = fill_levels("rpn_pyramid_decode", lv, y_host, nloc_host, A_host, ld_host, anchors_host, L, N, pre_nms_top_n, k_max, true);
    if (rc != ABR_OK) return rc;
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(idx && scores_in && img_hw && props && scores_out && counts, "rpn_pyramid_decode: null pointer");
    pyr_decode_kernel<<<(unsigned)(N * L), TT, 0, abr::as_stream(stream)>>>(lv, L, k_max, idx, scores_in, img_hw, wx, wy, ww, wh, min_size, props,
                                                                           scores_out, counts);
    ABR_CHECK_LAUNCH("rpn_pyramid_decode");
    return ABR_OK;
}

extern "C" int abr_rpn_pyramid_select(const float* props, const float* scores, const int32_t* keep, const int32_t* n_keep, int N, int L, int k_max,
                                      int post, int fpn_post_n, int mode, float* rois, float* out_scores, int32_t* src, int32_t* n_out,
                                      void* stream) {
    ABR_REQUIRE(L >= 1 && L <= MAXL, "rpn_pyramid_select: L = %d levels, need 1 .. %d", L, MAXL);
    ABR_REQUIRE(N >= 0 && k_max >= 1 && post >= 1 && fpn_post_n >= 1 && (mode == 0 || mode == 1), "rpn_pyramid_select: bad args");
    if (N == 0) return ABR_OK;
    const long long total = (long long)N * L * post;
    ABR_REQUIRE(total <= 0x7FFFFFFF && (long long)N * L * k_max * 4 <= 0x7FFFFFFF, "rpn_pyramid_select: N * L * post does not fit int32");
    const int cap = (int)std::min<long long>(fpn_post_n, (long long)L * post);
    ABR_REQUIRE(mode == 1 || cap <= SELCAP, "rpn_pyramid_select: %d proposals per image, the in-LDS sort of mode 0 holds %d", cap, SELCAP);
    ABR_REQUIRE(props && scores && keep && n_keep && rois && out_scores && src && n_out, "rpn_pyramid_select: null pointer");
    hipStream_t st = abr::as_stream(stream);
    const size_t wbytes = ((size_t)total * 8 + 63) & ~(size_t)63;
    char* b = static_cast<char*>(abr::scratch(abr::SCRATCH_RPN_SELECT, st, wbytes + (size_t)N * sizeof(SelThr)));
    ABR_REQUIRE(b, "rpn_pyramid_select: scratch allocation failed");
    unsigned long long* words = reinterpret_cast<unsigned long long*>(b);
    SelThr* thr = reinterpret_cast<SelThr*>(b + wbytes);
    sel_words_kernel<<<abr::cdiv(total, 256), 256, 0, st>>>(scores, keep, n_keep, (int)total, k_max, post, words);
    sel_threshold_kernel<<<mode ? 1 : N, TT, 0, st>>>(words, mode ? (int)total : L * post, fpn_post_n, thr);
    sel_emit_kernel<<<N, TT, 0, st>>>(words, thr, mode, L, k_max, post, cap, props, scores, keep, rois, out_scores, src, n_out);
    ABR_CHECK_LAUNCH("rpn_pyramid_select");
    return ABR_OK;
}
