// Ranking device code shared by topk.hip, rpn_pyramid.hip, detect.hip and retinanet.hip: score keys, 64-bit rank words, the radix-select step,
// the exact k-th word, the in-LDS bitonic sort and the stable in-order compaction.  Every ranking here orders by descending score and breaks ties by ascending index; the entry points agree on that, and on
// which elements tie, only while they share these definitions.
#pragma once
#include "common.h"

namespace abr {

// key of an objectness logit: the bit pattern of sigmoid(x) (rpn/inference.py:87-90 `.sigmoid()`; non-negative, so it orders like the value)
__device__ __forceinline__ unsigned sigmoid_key(float x) { return __float_as_uint(1.f / (1.f + expf(-x))); }

// key that orders like x itself for ANY finite float: sign bit flipped for x >= 0, all bits for x < 0 (-0 sorts below +0, NaNs at the ends)
__device__ __forceinline__ unsigned order_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// rank word: key in the high half, ~index in the low half -- unsigned order of the words = descending key, equal keys by ASCENDING index; words
// of distinct indices are distinct.  0 is free for padding whenever keys are non-zero.
__device__ __forceinline__ unsigned long long rank_word(unsigned key, unsigned index) { return ((unsigned long long)key << 32) | (unsigned)(~index); }
__device__ __forceinline__ unsigned rank_word_key(unsigned long long w) { return (unsigned)(w >> 32); }
__device__ __forceinline__ unsigned rank_word_index(unsigned long long w) { return ~(unsigned)(w & 0xFFFFFFFFu); }

// one radix-select step, by wave 0: the bin holding the s_krem-th largest element of histogram h (nbins a multiple of 64), counted from the TOP
// bin -> s_bin, s_krem -= what lies above it
__device__ __forceinline__ void find_bin_from_top(const int* h, int nbins, int* s_bin, int* s_krem) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x, per = nbins / 64;
        const int base_bin = (63 - lane) * per;          // lane 0 owns the top bins: a prefix scan over lanes is a suffix sum over bins
        int s = 0;
        for (int i = 0; i < per; i++) s += h[base_bin + i];
        int inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d, 64);
            if (lane >= d) inc += v;
        }
        const int exc = inc - s, krem = *s_krem;
        if (exc < krem && krem <= inc) {
            int cum = exc, b = base_bin + per - 1;
            for (; b > base_bin; b--) {
                if (cum + h[b] >= krem) break;
                cum += h[b];
            }
            *s_bin = b;
            *s_krem = krem - cum;
        }
    }
}

// descending bitonic sort of the words buf[0 .. p2) in LDS, p2 a power of two, by a whole workgroup of NT threads (all call; ends on a barrier)
template <int NT>
__device__ __forceinline__ void bitonic_desc(unsigned long long* buf, int p2) {
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll   // a constant p2 unrolls fully (topk_chunk_sort_kernel: two steps per thread); a run-time p2 stays a loop
            for (int t = threadIdx.x; t < (p2 >> 1); t += NT) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long x = buf[lo], y = buf[hi];
                if ((x < y) == desc) { buf[lo] = y; buf[hi] = x; }
            }
            __syncthreads();
        }
    }
}

// the want-th largest of the nonzero words a[0 .. m): six radix levels over all 64 bits (12, 12, 8 | 12, 12, 8); with first_level = 1 the top
// 12 bits are known to be `pre` already.  All threads call; h: 4096 ints of LDS.  Returns the word (valid when 1 <= want <= #nonzero words).
__device__ __forceinline__ unsigned long long kth_word(const unsigned long long* __restrict__ a, long long m, int want, int first_level,
                                                       unsigned long long pre, int* h, int* s_bin, int* s_krem) {
    if (threadIdx.x == 0) { *s_krem = want; *s_bin = 0; }
    __syncthreads();
    for (int lv = first_level; lv < 6; lv++) {
        const int sh = lv == 0 ? 52 : lv == 1 ? 40 : lv == 2 ? 32 : lv == 3 ? 20 : lv == 4 ? 8 : 0;
        const int bits = (lv == 2 || lv == 5) ? 8 : 12, nb = 1 << bits;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) h[i] = 0;
        __syncthreads();
        for (long long j = threadIdx.x; j < m; j += blockDim.x) {
            const unsigned long long w = a[j];
            if (w != 0ull && (lv == 0 || (w >> (sh + bits)) == pre)) atomicAdd(&h[(unsigned)(w >> sh) & (nb - 1)], 1);
        }
        __syncthreads();
        find_bin_from_top(h, nb, s_bin, s_krem);
        __syncthreads();
        pre = (pre << bits) | (unsigned)*s_bin;
        __syncthreads();
    }
    return pre;
}

// keep flag -> position among the workgroup's kept elements (rank order), running base in *s_base; all NT threads call; s_wave: NT / 64 ints of LDS
template <int NT>
__device__ __forceinline__ int compact_pos(bool keep, int* s_wave, int* s_base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = *s_base;
    for (int w = 0; w < wave; w++) off += s_wave[w];
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NT / 64; w++) t += s_wave[w];
        *s_base += t;
    }
    __syncthreads();
    return off + before;
}

}  // namespace abr
