// Instance-mask evaluation (VOC box and mask AP, evaluation/voc/voc_eval_inst.py) -- the mask side of masklist_iou
// (maskrcnn_benchmark/data/datasets/evaluation/voc/voc_eval_inst.py:89-105) as integer popcounts over bit-packed masks:
//   pack          [n,H,W] uint8 / fp32 -> [n,H,ceil(W/64)] 64-bit words, bit x % 64 of word x / 64 set iff mask == 1
//   resize + pack BinaryMaskList.resize (structures/segmentation_mask.py:113-135) of uint8 masks, fused: the resized image is never stored
//   pair counts   |pred & gt| for every (prediction, ground truth) pair of one image, and every mask's own area, in ONE launch
// A wave covers 64 consecutive pixels of a row and its ballot is the word (wave64, mask_out.h).  All three are memory-bound and short.
#include <algorithm>

#include "common.h"
#include "mask_bilinear.h"
#include "mask_out.h"

namespace {

constexpr int kPairChunk = 16;   // ground truths whose counts one thread keeps in registers per pass over its predicted words

// the pixel predicates of the two packers (mask_out.h)
template <typename T>
struct PackPixel {
    const T* masks;
    int H, W;
    __device__ __forceinline__ void instance(long long) {}
    __device__ __forceinline__ bool operator()(long long i, int y, int x) const { return masks[(i * H + y) * W + x] == (T)1; }
};

// a destination pixel: the truncated bilinear sample of the source compared with 1
struct ResizePixel {
    const uint8_t* masks;
    int Hs, Ws;
    float sh, sw;
    int four_weight;
    __device__ __forceinline__ void instance(long long) {}
    __device__ __forceinline__ bool operator()(long long i, int y, int x) const {
        int y0, y1, x0, x1;
        float ly, lx;
        bilinear_tap(sh, y, Hs, y0, y1, ly);
        bilinear_tap(sw, x, Ws, x0, x1, lx);
        const uint8_t* m = masks + i * Hs * Ws;
        const uint8_t* r0 = m + (int64_t)y0 * Ws;
        const uint8_t* r1 = m + (int64_t)y1 * Ws;
        const float v00 = (float)r0[x0], v01 = (float)r0[x1], v10 = (float)r1[x0], v11 = (float)r1[x1];
        const float v = four_weight ? bilinear_mix(v00, v01, v10, v11, lx, ly) : bilinear_mix_separable(v00, v01, v10, v11, lx, ly);
        return (unsigned char)(int)v == 1;     // .type_as(uint8 masks) truncates, then masklist_iou's == 1
    }
};

template <typename T>
__global__ __launch_bounds__(256) void mask_pack_bits_kernel(const T* __restrict__ masks, int64_t n_words, int H, int W, int Wq,
                                                             unsigned long long* __restrict__ bits) {
    abr::mask_write_bits(PackPixel<T>{masks, H, W}, n_words, H, W, Wq, bits);
}

__global__ __launch_bounds__(256) void mask_resize_pack_bits_kernel(const uint8_t* __restrict__ masks, int64_t n_words, int Hs, int Ws, int Hd,
                                                                    int Wd, int Wq, float sh, float sw, int four_weight,
                                                                    unsigned long long* __restrict__ bits) {
    abr::mask_write_bits(ResizePixel{masks, Hs, Ws, sh, sw, four_weight}, n_words, Hd, Wd, Wq, bits);
}

__device__ __forceinline__ int block_sum_int(int v, int* s4) {   // 256 threads; every thread returns the total
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// blocks [0,P): prediction p against every ground truth, its words read once per chunk of kPairChunk ground truths (once for T <= 16);
// blocks [P,P+T): the area of ground truth b - P.  Pairs whose labels differ are never read.
__global__ __launch_bounds__(256) void mask_pair_counts_kernel(const unsigned long long* __restrict__ pred, const unsigned long long* __restrict__ gt,
                                                               const int64_t* __restrict__ pred_labels, const int64_t* __restrict__ gt_labels, int P,
                                                               int T, int64_t words, int32_t* __restrict__ inter, int32_t* __restrict__ area_p,
                                                               int32_t* __restrict__ area_t) {
    __shared__ int s4[4];
    const int b = blockIdx.x;
    if (b >= P) {
        const unsigned long long* g = gt + (int64_t)(b - P) * words;
        int a = 0;
        for (int64_t i = threadIdx.x; i < words; i += 256) a += __popcll(g[i]);
        a = block_sum_int(a, s4);
        if (threadIdx.x == 0) area_t[b - P] = a;
        return;
    }
    const unsigned long long* pw = pred + (int64_t)b * words;
    const bool labelled = pred_labels != nullptr && gt_labels != nullptr;
    const int64_t pl = labelled ? pred_labels[b] : 0;
    for (int t0 = 0; t0 < T; t0 += kPairChunk) {
        const int nt = min(kPairChunk, T - t0);
        bool live[kPairChunk];
        int acc[kPairChunk];
        int area = 0;
#pragma unroll
        for (int j = 0; j < kPairChunk; j++) {
            acc[j] = 0;
            live[j] = j < nt && (!labelled || gt_labels[t0 + j] == pl);      // (block-uniform)
        }
        for (int64_t i = threadIdx.x; i < words; i += 256) {
            const unsigned long long w = pw[i];
            area += __popcll(w);
#pragma unroll
            for (int j = 0; j < kPairChunk; j++)
                if (live[j]) acc[j] += __popcll(w & gt[(int64_t)(t0 + j) * words + i]);
        }
#pragma unroll
        for (int j = 0; j < kPairChunk; j++) {
            if (j < nt) {                                                  // (block-uniform: block_sum_int synchronises)
                const int v = live[j] ? block_sum_int(acc[j], s4) : 0;
                if (threadIdx.x == 0) inter[(int64_t)b * T + t0 + j] = v;
            }
        }
        if (t0 == 0) {
            area = block_sum_int(area, s4);
            if (threadIdx.x == 0) area_p[b] = area;
        }
    }
}

bool image_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }

}  // namespace

extern "C" int abr_mask_pack_bits(const void* masks, int is_u8, int n, int H, int W, uint64_t* bits, void* stream) {
    ABR_REQUIRE(n >= 0 && image_ok(H, W), "mask_pack_bits: bad args (n >= 0, 0 < H * W < 2^31)");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(masks && bits, "mask_pack_bits: null pointer");
    const int Wq = (W + 63) / 64;
    const int64_t n_words = (int64_t)n * H * Wq;
    hipStream_t st = abr::as_stream(stream);
    auto* out = reinterpret_cast<unsigned long long*>(bits);
    if (is_u8)
        mask_pack_bits_kernel<uint8_t><<<abr::wave_grid(n_words), 256, 0, st>>>(static_cast<const uint8_t*>(masks), n_words, H, W, Wq, out);
    else
        mask_pack_bits_kernel<float><<<abr::wave_grid(n_words), 256, 0, st>>>(static_cast<const float*>(masks), n_words, H, W, Wq, out);
    ABR_CHECK_LAUNCH("mask_pack_bits");
    return ABR_OK;
}

extern "C" int abr_mask_resize_pack_bits(const uint8_t* masks, int n, int Hs, int Ws, int Hd, int Wd, uint64_t* bits, void* stream) {
    ABR_REQUIRE(n >= 0 && image_ok(Hs, Ws) && image_ok(Hd, Wd), "mask_resize_pack_bits: bad args (n >= 0, 0 < H * W < 2^31 for both sizes)");
    if (Hs == Hd && Ws == Wd) return abr_mask_pack_bits(masks, 1, n, Hd, Wd, bits, stream);
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(masks && bits, "mask_resize_pack_bits: null pointer");
    const int Wq = (Wd + 63) / 64;
    const int64_t n_words = (int64_t)n * Hd * Wq;
    // area_pixel_compute_scale: float(input) / output
    mask_resize_pack_bits_kernel<<<abr::wave_grid(n_words), 256, 0, abr::as_stream(stream)>>>(masks, n_words, Hs, Ws, Hd, Wd, Wq, (float)Hs / (float)Hd,
                                                                                       (float)Ws / (float)Wd, bilinear_four_weight_path(Hd, Wd) ? 1 : 0,
                                                                                       reinterpret_cast<unsigned long long*>(bits));
    ABR_CHECK_LAUNCH("mask_resize_pack_bits");
    return ABR_OK;
}

extern "C" int abr_mask_pair_counts(const uint64_t* pred_bits, const uint64_t* gt_bits, const int64_t* pred_labels, const int64_t* gt_labels, int P,
                                    int T, int H, int W, int64_t words, int32_t* inter, int32_t* area_p, int32_t* area_t, void* stream) {
    ABR_REQUIRE(P >= 0 && T >= 0 && image_ok(H, W), "mask_pair_counts: bad args (P, T >= 0, 0 < H * W < 2^31)");
    ABR_REQUIRE(words == (int64_t)H * ((W + 63) / 64), "mask_pair_counts: words is not H * ceil(W / 64)");
    ABR_REQUIRE((P == 0 || (pred_bits && area_p)) && (T == 0 || (gt_bits && area_t)) && (P == 0 || T == 0 || inter), "mask_pair_counts: null pointer");
    ABR_REQUIRE((pred_labels == nullptr) == (gt_labels == nullptr) || P == 0 || T == 0, "mask_pair_counts: labels must be given for both sides or neither");
    if (P == 0 || T == 0) return ABR_OK;
    mask_pair_counts_kernel<<<P + T, 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const unsigned long long*>(pred_bits),
                                                                      reinterpret_cast<const unsigned long long*>(gt_bits), pred_labels, gt_labels, P, T,
                                                                      words, inter, area_p, area_t);
    ABR_CHECK_LAUNCH("mask_pair_counts");
    return ABR_OK;
}
