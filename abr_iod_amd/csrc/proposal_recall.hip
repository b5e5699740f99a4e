// Proposal recall (evaluation/coco/coco_eval.py: evaluate_box_proposals): the greedy cover of an image's ground truths
// by its ranked proposals, for every image x proposal limit x area range of a dataset in ONE launch.
// A CELL is one (image, limit, area range): the image's first min(P, limit) proposals against its ground truths whose area lies in the
// range.  The reference takes, min(P, G) times, the largest remaining entry of the P x G IoU matrix (ties: the lowest ground truth, then
// the lowest proposal rank -- Tensor.max's first maximal index), records it and strikes its row and column.
// Arrangement: one wave per cell, nothing of the matrix is kept.  Every ground truth holds its best remaining proposal as (value, rank) in
// a register of its owner lane (ground truth j: lane j & 63, slot j >> 6); a round is an arg-max over those (max value, min ground truth),
// and only the ground truths whose best WAS the struck proposal scan the proposals again.  A scan is wave-cooperative: lane l reads
// proposals l, l + 64, ... from LDS and the lanes reduce on (max value, min rank).  The struck proposals are one bit per proposal in the
// lane that scans it.  The cells of an image do not share IoUs: a cell is its own workgroup (16 KB of boxes + 2.5 KB of state in LDS).
// The IoU is boxlist_iou's float32 arithmetic, one rounding per operation (contraction off): bit for bit the host restatement's.
#include "common.h"

#include <climits>

namespace {

constexpr int kMaxGt = ABR_COCO_MATCH_MAX_GT;
constexpr int kMaxProp = ABR_PROPOSAL_COVER_MAX_PROP;
constexpr int kMaxThr = 16;
static_assert(kMaxGt == 128 && kMaxProp == 1024, "two ground-truth slots per lane, one struck bit per proposal in a 16-bit field per lane");

struct Best {
    float v;
    int r;
};

// (max value, min index) over the wave; every lane leaves with the same pair
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(b.v, off, 64);
        const int orr = __shfl_xor(b.r, off, 64);
        if (ov > b.v || (ov == b.v && orr < b.r)) {
            b.v = ov;
            b.r = orr;
        }
    }
    return b;
}

__device__ __forceinline__ float box_area1(const float4 b) {
#pragma clang fp contract(off)
    return (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
}

__device__ __forceinline__ float cover_iou(const float4 p, const float4 g, const float ga) {
#pragma clang fp contract(off)
    const float pa = (p.z - p.x + 1.f) * (p.w - p.y + 1.f);
    const float w = fmaxf(fminf(p.z, g.z) - fmaxf(p.x, g.x) + 1.f, 0.f);
    const float h = fmaxf(fminf(p.w, g.w) - fmaxf(p.y, g.y) + 1.f, 0.f);
    const float inter = w * h;
    return inter / (pa + ga - inter);
}

// the best proposal left for ground truth g: lane l looks at proposals l, l + 64, ... (bit k of `struck`: proposal l + 64 k is gone)
__device__ __forceinline__ Best scan_proposals(const float4* s_prop, int P, unsigned struck, const float4 g, int lane) {
    const float ga = box_area1(g);
    Best b{-1.f, INT_MAX};
    for (int k = 0, p = lane; p < P; k++, p += 64) {
        if ((struck >> k) & 1u) continue;
        const float v = cover_iou(s_prop[p], g, ga);
        if (v > b.v) {       // (ranks ascend: the first maximum stays)
            b.v = v;
            b.r = p;
        }
    }
    return wave_best(b);
}

__global__ __launch_bounds__(64) void proposal_cover_kernel(const float4* __restrict__ prop, const float4* __restrict__ gt,
                                                            const float* __restrict__ gt_area, const int64_t* __restrict__ prop_off,
                                                            const int64_t* __restrict__ gt_off, const float* __restrict__ area_rng, int A,
                                                            const int32_t* __restrict__ limits, const float* __restrict__ thrs, int T,
                                                            int64_t g_total, float* __restrict__ overlaps, int32_t* __restrict__ hits,
                                                            int32_t* __restrict__ num_pos, int32_t* __restrict__ n_over) {
    __shared__ float4 s_prop[kMaxProp];
    __shared__ float4 s_gt[kMaxGt];        // the ground truths of the range, in file order
    __shared__ float s_rec[kMaxGt];        // the recorded overlaps, in round order
    __shared__ int s_hits[kMaxThr];
    const int img = blockIdx.x, cell = blockIdx.y, lane = threadIdx.x;
    const int l = cell / A, a = cell % A;
    const int64_t p0 = prop_off[img], g0 = gt_off[img];
    const int64_t P_img = prop_off[img + 1] - p0, G64 = gt_off[img + 1] - g0;
    if (G64 <= 0) return;                  // (the reference skips an image without a non-crowd ground truth)
    if (P_img > kMaxProp || G64 > kMaxGt) {        // (block-uniform) left to the host, whole
        if (cell == 0 && lane == 0) atomicAdd(n_over, 1);
        return;
    }
    const int G = (int)G64;
    const float lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    int Gv = 0;
    for (int base = 0; base < G; base += 64) {
        const int g = base + lane;
        bool in = false;
        if (g < G) {
            const float ar = gt_area[g0 + g];
            in = ar >= lo && ar <= hi;
        }
        const unsigned long long m = __ballot(in);
        if (in) s_gt[Gv + __popcll(m & ((1ull << lane) - 1ull))] = gt[g0 + g];
        Gv += __popcll(m);
    }
    if (l == 0 && lane == 0 && Gv > 0) atomicAdd(&num_pos[a], Gv);
    float* out = overlaps + (int64_t)cell * g_total + g0;
    const int lim = limits[l];
    const int P = (int)(P_img < (int64_t)lim ? P_img : (int64_t)lim);
    if (Gv == 0 || P <= 0) {               // no vector: the reference appends nothing for this image
        for (int g = lane; g < G; g += 64) out[g] = -1.f;
        return;
    }
    for (int p = lane; p < P; p += 64) s_prop[p] = prop[p0 + p];
    if (lane < kMaxThr) s_hits[lane] = 0;
    __syncthreads();

    float bv0 = -1.f, bv1 = -1.f;
    int br0 = INT_MAX, br1 = INT_MAX;
    unsigned struck = 0u;
    for (int j = 0; j < Gv; j++) {
        const Best b = scan_proposals(s_prop, P, struck, s_gt[j], lane);
        if (lane == (j & 63)) {
            if (j < 64) { bv0 = b.v; br0 = b.r; } else { bv1 = b.v; br1 = b.r; }
        }
    }
    bool alive0 = lane < Gv, alive1 = lane + 64 < Gv;
    const int rounds = P < Gv ? P : Gv;
    for (int i = 0; i < rounds; i++) {
        Best c{-1.f, INT_MAX};
        if (alive0) { c.v = bv0; c.r = lane; }
        if (alive1 && bv1 > c.v) { c.v = bv1; c.r = lane + 64; }
        c = wave_best(c);
        const int jstar = c.r;             // (a live pair exists in every round: min(P, Gv) rounds)
        const int pstar = __shfl(jstar < 64 ? br0 : br1, jstar & 63, 64);
        if (lane == 0) s_rec[i] = c.v;
        if (lane == (jstar & 63)) {
            if (jstar < 64) alive0 = false; else alive1 = false;
        }
        // (pstar == INT_MAX: every overlap left for that ground truth is NaN, boxes with x2 < x1; -1 is recorded and no proposal retires)
        if (pstar != INT_MAX && lane == (pstar & 63)) struck |= 1u << (pstar >> 6);
        if (i + 1 == rounds) break;
        unsigned long long m0 = __ballot(alive0 && br0 == pstar), m1 = __ballot(alive1 && br1 == pstar);
        while (m0) {
            const int ln = __ffsll((long long)m0) - 1;
            m0 &= m0 - 1ull;
            const Best b = scan_proposals(s_prop, P, struck, s_gt[ln], lane);
            if (lane == ln) { bv0 = b.v; br0 = b.r; }
        }
        while (m1) {
            const int ln = __ffsll((long long)m1) - 1;
            m1 &= m1 - 1ull;
            const Best b = scan_proposals(s_prop, P, struck, s_gt[ln + 64], lane);
            if (lane == ln) { bv1 = b.v; br1 = b.r; }
        }
    }
    __syncthreads();
    for (int g = lane; g < G; g += 64) {
        const float v = g < rounds ? s_rec[g] : (g < Gv ? 0.f : -1.f);
        out[g] = v;
        if (g < Gv)
            for (int t = 0; t < T; t++)
                if (v >= thrs[t]) atomicAdd(&s_hits[t], 1);
    }
    __syncthreads();
    if (lane < T && s_hits[lane] > 0) atomicAdd(&hits[cell * T + lane], s_hits[lane]);
}

}  // namespace

extern "C" int abr_proposal_cover_max_prop(void) { return kMaxProp; }

extern "C" int abr_proposal_cover(const float* prop, const float* gt, const float* gt_area, const int64_t* prop_off, const int64_t* gt_off,
                                  int n_images, int64_t p_total, int64_t g_total, const float* area_rng, int A, const int32_t* limits, int L,
                                  const float* thrs, int T, float* overlaps, int32_t* hits, int32_t* num_pos, int32_t* n_over, void* stream) {
    ABR_REQUIRE(n_images >= 0 && p_total >= 0 && g_total >= 0, "proposal_cover: bad args (n_images, p_total, g_total >= 0)");
    ABR_REQUIRE(A >= 1 && A <= 8 && L >= 1 && L <= 4 && T >= 1 && T <= kMaxThr, "proposal_cover: bad args (1 <= A <= 8, 1 <= L <= 4, 1 <= T <= 16)");
    if (n_images == 0 || g_total == 0) return ABR_OK;      // no ground truth anywhere: nothing to write, num_pos stays as zeroed
    ABR_REQUIRE(gt && gt_area && prop_off && gt_off && area_rng && limits && thrs && overlaps && hits && num_pos && n_over && (p_total == 0 || prop),
                "proposal_cover: null pointer");
    ABR_REQUIRE((reinterpret_cast<uintptr_t>(prop) & 15) == 0 && (reinterpret_cast<uintptr_t>(gt) & 15) == 0,
                "proposal_cover: prop and gt must be 16-byte aligned (rows are read whole)");
    proposal_cover_kernel<<<dim3(n_images, L * A), 64, 0, abr::as_stream(stream)>>>(
        reinterpret_cast<const float4*>(prop), reinterpret_cast<const float4*>(gt), gt_area, prop_off, gt_off, area_rng, A, limits, thrs, T, g_total,
        overlaps, hits, num_pos, n_over);
    ABR_CHECK_LAUNCH("proposal_cover");
    return ABR_OK;
}
