// The two ways an instance-mask kernel writes its [n,h,w] result, once: the packed words of abr_mask_pack_bits (mask_eval.hip's pack and
// resize + pack, rle.hip's and poly.hip's packed outputs) and the row-major uint8 bytes (rle.hip's and poly.hip's byte outputs).  A kernel
// differs only in how a pixel is decided, which it hands over as a PREDICATE:
//     void instance(long long k)                  called before the pixels of instance k are asked for: fetch what belongs to the instance
//     bool operator()(long long k, int y, int x)  is pixel (y, x) of instance k set?  (0 <= y < h, 0 <= x < w)
#pragma once
#include <algorithm>

#include "common.h"

namespace abr {

__host__ __device__ __forceinline__ long long clamp64(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Packed words [n,h,Wq = ceil(w/64)]: bit x % 64 of word x / 64 of a row is pixel x, bits past w are zero.  A wave per word: lane = pixel, the
// wave's ballot = the word, lane 0 stores it.  Workgroups of 256 threads, grid-stride over the words (wave_grid); everything but x is
// wave-uniform, and instance() is called once per word.
template <typename Pred>
__device__ __forceinline__ void mask_write_bits(Pred pred, long long n_words, int h, int w, int Wq, unsigned long long* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long wd = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); wd < n_words; wd += n_waves) {     // (wave-uniform)
        const int q = (int)(wd % Wq);
        const long long row = wd / Wq;          // = k * h + y
        const int y = (int)(row % h);
        const long long k = row / h;
        Pred p = pred;      // (what instance() fetches lives for one word)
        p.instance(k);
        const int x = q * 64 + lane;
        const bool set = x < w && p(k, y, x);
        const unsigned long long word = __ballot(set);
        if (lane == 0) bits[wd] = word;
    }
}
inline unsigned wave_grid(int64_t n_words) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_words + 3) / 4, 16384)); }

// Bytes [n,h,w] of 0 / 1 (`out` 4-byte aligned): 4 consecutive bytes of the flat output per thread, one dword store; the (numel % 4) tail bytes
// one by one by the last thread.  A quad may straddle instances: instance() is called when k changes within it.  Workgroups of 256 threads,
// grid-stride over the quads.
template <typename Pred>
__device__ __forceinline__ void mask_write_u8(Pred pred, long long numel, int h, int w, uint8_t* __restrict__ out) {
    const long long hw = (long long)h * w;
    const long long n_quads = (numel + 3) / 4;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n_quads; t += (long long)gridDim.x * 256) {
        uint32_t word = 0;
        const long long f0 = t * 4;
        long long k_prev = -1;
        Pred p = pred;      // (what instance() fetches lives for one quad)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const long long f = f0 + q;
            if (f >= numel) break;
            const long long k = f / hw;
            if (k != k_prev) { p.instance(k); k_prev = k; }
            const int rem = (int)(f - k * hw);
            const int y = rem / w, x = rem - y * w;
            word |= (uint32_t)p(k, y, x) << (8 * q);
        }
        if (f0 + 4 <= numel) *reinterpret_cast<uint32_t*>(out + f0) = word;
        else for (int q = 0; f0 + q < numel; q++) out[f0 + q] = (uint8_t)(word >> (8 * q));
    }
}
inline unsigned quad_grid(int64_t numel) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((numel / 4 + 256) / 256, 65536)); }

}  // namespace abr
