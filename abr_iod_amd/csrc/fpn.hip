// The neck of a feature pyramid network (modeling/backbone/fpn.py): the top-down pathway, forward and backward, in one launch each, and
// LastLevelMaxPool (a stride-2 subsample) with its backward.  All HBM-bound: NHWC fp32 maps, one float4 (16 B) per lane along C so that a wave
// covers 1 KB of consecutive channels of one pixel, no LDS, no atomics.
//
// The reference walks the levels from the top: per level an F.interpolate (one launch, one map written and read back) and an add (another).
// Here an output element re-reads its coarser ancestors instead of waiting for them: the L-1 dependent launch pairs become one launch, at the
// price of at most 1/4 + 1/16 + ... = 1/3 more reads, nearly all of them L2 hits (four neighbours share every ancestor).  The level tables
// travel by value in the kernel arguments, as roi_align.hip's pyramid kernels pass theirs.  Every level choice below is a compile-time index
// into those tables behind a workgroup-uniform condition: scalar loads from the kernel arguments, no private copy of the table.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kMaxL = ABR_MAX_PYRAMID_LEVELS;

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

struct FpnFwd {
    const float4* lat[kMaxL];
    float4* inner[kMaxL];
    int H[kMaxL], W[kMaxL];
    unsigned first_block[kMaxL];   // of output level l (l < L-1); levels own whole workgroups, so the level is uniform in a workgroup
};

// one thread per float4 of inner_0 .. inner_{L-2}
__global__ __launch_bounds__(256) void fpn_topdown_fwd(FpnFwd t, int L, int B, int C4) {
    int l = 0, H = t.H[0], W = t.W[0];
    unsigned first = 0;
    float4* out = t.inner[0];
#pragma unroll
    for (int k = 1; k < kMaxL - 1; k++)
        if (k < L - 1 && blockIdx.x >= t.first_block[k]) { l = k; H = t.H[k]; W = t.W[k]; first = t.first_block[k]; out = t.inner[k]; }
    const int64_t i = (int64_t)(blockIdx.x - first) * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W * C4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H), b = (int)(p / H);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = kMaxL - 1; j >= 0; j--) {   // from the top level down to l, the reference's order of additions
        if (j > L - 1 || j < l) continue;
        const int s = j - l;
        const float4 a = t.lat[j][(((size_t)b * t.H[j] + (y >> s)) * t.W[j] + (x >> s)) * C4 + c];
        v = j == L - 1 ? a : add4(a, v);
    }
    out[i] = v;
}

struct FpnBwd {
    const float4* g[kMaxL];   // g[l] == nullptr (l >= 1): no gradient arrives at inner_l
    float4* d[kMaxL];
    int H[kMaxL], W[kMaxL];
};

// One thread per (image, pixel of the coarsest level, 4 channels) folds the 4^(L-1) finest pixels below it in Morton order, a level-1 node (its
// four level-0 children and g_1: five loads in flight) per iteration; s0 / s1 hold, per level, the sums of the first and second pair of
// children that have completed: T = g + ((c00 + c01) + (c10 + c11)).  d[l] may be g[l]: a thread reads an element only before it writes it.
template <int L>
__global__ __launch_bounds__(256) void fpn_topdown_bwd(FpnBwd t, int B, int C4) {
    static_assert(L >= 2 && L <= kMaxL, "levels");
    const int Ht = t.H[L - 1], Wt = t.W[L - 1];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Ht * Wt * C4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int X = (int)(p % Wt);
    p /= Wt;
    const int Y = (int)(p % Ht), b = (int)(p / Ht);
    const int H0 = t.H[0], W0 = t.W[0], H1 = t.H[1], W1 = t.W[1];
    const float4* g0 = t.g[0];
    const float4* g1 = t.g[1];
    float4* d0 = t.d[0];
    float4* d1 = t.d[1];
    const bool write0 = d0 != g0;
    float4 s0[L], s1[L];
#pragma unroll
    for (int l = 0; l < L; l++) s0[l] = s1[l] = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int NQ = 1 << (2 * (L - 2));
    for (int j = 0; j < NQ; j++) {
        int dy = 0, dx = 0;
#pragma unroll
        for (int k = 0; k < L - 2; k++) {
            dx |= ((j >> (2 * k)) & 1) << k;
            dy |= ((j >> (2 * k + 1)) & 1) << k;
        }
        const int y1 = (Y << (L - 2)) + dy, x1 = (X << (L - 2)) + dx;
        const size_t r0 = (((size_t)b * H0 + 2 * y1) * W0 + 2 * x1) * C4 + c, row = (size_t)W0 * C4;
        const size_t i1 = (((size_t)b * H1 + y1) * W1 + x1) * C4 + c;
        const float4 c00 = g0[r0], c01 = g0[r0 + C4], c10 = g0[r0 + row], c11 = g0[r0 + row + C4];
        float4 v = add4(add4(c00, c01), add4(c10, c11));
        if (g1) v = add4(g1[i1], v);
        if (write0) {
            d0[r0] = c00;
            d0[r0 + C4] = c01;
            d0[r0 + row] = c10;
            d0[r0 + row + C4] = c11;
        }
        d1[i1] = v;
        bool up = true;   // v = a completed node of level l-1: hand it to its parent on level l
#pragma unroll
        for (int l = 2; l < L; l++) {
            if (!up) continue;
            const int k = (j >> (2 * (l - 2))) & 3;
            if (k == 0) s0[l] = v;
            else if (k == 1) s0[l] = add4(s0[l], v);
            else if (k == 2) s1[l] = v;
            else {
                v = add4(s0[l], add4(s1[l], v));
                const size_t il = (((size_t)b * t.H[l] + (y1 >> (l - 1))) * t.W[l] + (x1 >> (l - 1))) * C4 + c;
                if (t.g[l]) v = add4(t.g[l][il], v);
                t.d[l][il] = v;
            }
            up = k == 3;
        }
    }
}

__global__ __launch_bounds__(256) void fpn_copy(const float4* g, float4* d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = g[i];
}

__global__ __launch_bounds__(256) void fpn_subsample2_fwd(const float4* __restrict__ x, int B, int H, int W, int Ho, int Wo, int C4,
                                                           float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Ho * Wo * C4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int xo = (int)(p % Wo);
    p /= Wo;
    const int yo = (int)(p % Ho), b = (int)(p / Ho);
    out[i] = x[(((size_t)b * H + 2 * yo) * W + 2 * xo) * C4 + c];
}

// g_x may be g_in: every element is read and written by the same thread
__global__ __launch_bounds__(256) void fpn_subsample2_bwd(const float4* __restrict__ g_out, const float4* g_in, int B, int H, int W, int Ho, int Wo,
                                                           int C4, float4* g_x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W * C4) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H), b = (int)(p / H);
    float4 v = g_in ? g_in[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (((x | y) & 1) == 0) {
        const float4 g = g_out[(((size_t)b * Ho + (y >> 1)) * Wo + (x >> 1)) * C4 + c];
        v = g_in ? add4(v, g) : g;
    }
    g_x[i] = v;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks the two top-down entry points share
int check_levels(const char* name, const int* H, const int* W, int L, int B, int C) {
    ABR_REQUIRE(L >= 1 && L <= kMaxL, "%s: L = %d levels, need 1 .. %d", name, L, kMaxL);
    ABR_REQUIRE(H && W, "%s: null level table", name);
    ABR_REQUIRE(B > 0 && C > 0 && C % 4 == 0, "%s: B = %d, C = %d: need B > 0 and C a positive multiple of 4", name, B, C);
    for (int l = 0; l < L; l++) ABR_REQUIRE(H[l] >= 1 && W[l] >= 1, "%s: level %d is %d x %d", name, l, H[l], W[l]);
    for (int l = 0; l + 1 < L; l++)
        ABR_REQUIRE(H[l] == 2 * H[l + 1] && W[l] == 2 * W[l + 1], "%s: level %d is %d x %d, not twice level %d's %d x %d", name, l, H[l], W[l],
                    l + 1, H[l + 1], W[l + 1]);
    ABR_REQUIRE((int64_t)B * H[0] * W[0] * (C / 4) <= INT32_MAX, "%s: B * H[0] * W[0] * C / 4 does not fit int32", name);
    return ABR_OK;
}

template <int L>
void launch_bwd(const FpnBwd& t, int B, int C4, hipStream_t st) {
    const int64_t n = (int64_t)B * t.H[L - 1] * t.W[L - 1] * C4;
    fpn_topdown_bwd<L><<<abr::cdiv(n, 256), 256, 0, st>>>(t, B, C4);
}

}  // namespace

extern "C" int abr_fpn_topdown_forward(const float* const* lat, float* const* inner, const int* H, const int* W, int L, int B, int C, void* stream) {
    const int rc = check_levels("fpn_topdown_forward", H, W, L, B, C);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(lat && inner, "fpn_topdown_forward: null pointer table");
    for (int l = 0; l < L; l++) {
        ABR_REQUIRE(lat[l] && aligned16(lat[l]), "fpn_topdown_forward: lateral %d is null or not 16-byte aligned", l);
        if (l < L - 1) {
            ABR_REQUIRE(inner[l] && aligned16(inner[l]), "fpn_topdown_forward: output %d is null or not 16-byte aligned", l);
            for (int j = 0; j < L; j++) ABR_REQUIRE(inner[l] != lat[j], "fpn_topdown_forward: output %d aliases lateral %d", l, j);
        }
    }
    if (L == 1) return ABR_OK;
    FpnFwd t{};
    const int C4 = C / 4;
    int64_t blocks = 0;
    for (int l = 0; l < L; l++) {
        t.lat[l] = reinterpret_cast<const float4*>(lat[l]);
        t.inner[l] = l < L - 1 ? reinterpret_cast<float4*>(inner[l]) : nullptr;
        t.H[l] = H[l];
        t.W[l] = W[l];
        t.first_block[l] = (unsigned)blocks;
        if (l < L - 1) blocks += abr::cdiv((int64_t)B * H[l] * W[l] * C4, 256);
    }
    fpn_topdown_fwd<<<(unsigned)blocks, 256, 0, abr::as_stream(stream)>>>(t, L, B, C4);
    ABR_CHECK_LAUNCH("fpn_topdown_forward");
    return ABR_OK;
}

extern "C" int abr_fpn_topdown_backward(const float* const* g, float* const* d_lat, const int* H, const int* W, int L, int B, int C, void* stream) {
    const int rc = check_levels("fpn_topdown_backward", H, W, L, B, C);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(g && d_lat, "fpn_topdown_backward: null pointer table");
    ABR_REQUIRE(g[0], "fpn_topdown_backward: the finest level's gradient is null");
    FpnBwd t{};
    for (int l = 0; l < L; l++) {
        ABR_REQUIRE(aligned16(g[l]), "fpn_topdown_backward: gradient %d is not 16-byte aligned", l);
        ABR_REQUIRE(d_lat[l] && aligned16(d_lat[l]), "fpn_topdown_backward: output %d is null or not 16-byte aligned", l);
        for (int j = 0; j < L; j++) ABR_REQUIRE(j == l || d_lat[l] != g[j], "fpn_topdown_backward: output %d aliases gradient %d", l, j);
        t.g[l] = reinterpret_cast<const float4*>(g[l]);
        t.d[l] = reinterpret_cast<float4*>(d_lat[l]);
        t.H[l] = H[l];
        t.W[l] = W[l];
    }
    hipStream_t st = abr::as_stream(stream);
    const int C4 = C / 4;
    switch (L) {
        case 1: {
            if (d_lat[0] == g[0]) return ABR_OK;
            const int64_t n = (int64_t)B * H[0] * W[0] * C4;
            fpn_copy<<<abr::cdiv(n, 256), 256, 0, st>>>(t.g[0], t.d[0], n);
            break;
        }
        case 2: launch_bwd<2>(t, B, C4, st); break;
        case 3: launch_bwd<3>(t, B, C4, st); break;
        case 4: launch_bwd<4>(t, B, C4, st); break;
        case 5: launch_bwd<5>(t, B, C4, st); break;
        case 6: launch_bwd<6>(t, B, C4, st); break;
        case 7: launch_bwd<7>(t, B, C4, st); break;
        default: launch_bwd<8>(t, B, C4, st); break;
    }
    ABR_CHECK_LAUNCH("fpn_topdown_backward");
    return ABR_OK;
}

extern "C" int abr_fpn_subsample2_forward(const float* x, int B, int H, int W, int C, float* out, void* stream) {
    ABR_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "fpn_subsample2_forward: B = %d, H = %d, W = %d, C = %d: need positive sizes and C %% 4 == 0",
                B, H, W, C);
    ABR_REQUIRE((int64_t)B * H * W * (C / 4) <= INT32_MAX, "fpn_subsample2_forward: B * H * W * C / 4 does not fit int32");
    ABR_REQUIRE(x && out && aligned16(x) && aligned16(out), "fpn_subsample2_forward: null or misaligned pointer");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, C4 = C / 4;
    fpn_subsample2_fwd<<<abr::cdiv((int64_t)B * Ho * Wo * C4, 256), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(x), B, H, W, Ho, Wo, C4,
                                                                                                       reinterpret_cast<float4*>(out));
    ABR_CHECK_LAUNCH("fpn_subsample2_forward");
    return ABR_OK;
}

extern "C" int abr_fpn_subsample2_backward(const float* g_out, const float* g_in, int B, int H, int W, int C, float* g_x, void* stream) {
    ABR_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "fpn_subsample2_backward: B = %d, H = %d, W = %d, C = %d: need positive sizes and C %% 4 == 0",
                B, H, W, C);
    ABR_REQUIRE((int64_t)B * H * W * (C / 4) <= INT32_MAX, "fpn_subsample2_backward: B * H * W * C / 4 does not fit int32");
    ABR_REQUIRE(g_out && g_x && aligned16(g_out) && aligned16(g_x) && aligned16(g_in), "fpn_subsample2_backward: null or misaligned pointer");
    ABR_REQUIRE(g_x != g_out, "fpn_subsample2_backward: g_x aliases g_out");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, C4 = C / 4;
    fpn_subsample2_bwd<<<abr::cdiv((int64_t)B * H * W * C4, 256), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(g_out),
                                                                                                     reinterpret_cast<const float4*>(g_in), B, H, W, Ho, Wo,
                                                                                                     C4, reinterpret_cast<float4*>(g_x));
    ABR_CHECK_LAUNCH("fpn_subsample2_backward");
    return ABR_OK;
}
