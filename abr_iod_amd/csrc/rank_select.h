// Ranking device code shared by topk.hip, rpn_pyramid.hip and detect.hip: score keys, 64-bit rank words, the radix-select step and the in-LDS
// bitonic sort.  Every ranking here orders by descending score and breaks ties by ascending index; the entry points agree on that, and on
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

}  // namespace abr
