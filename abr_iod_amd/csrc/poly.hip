// Polygon instance masks on the device (include/abr_iod_hip.h section 12): the scan conversion pycocotools' rleFrPoly + merge + decode
// perform, restated from the algorithm (nothing here was compared with pycocotools, which this project cannot run).
//   one polygon of k vertices on an h x w grid, everything in double with C (int) casts:
//     X[j] = (int)(5 x[j] + .5), Y likewise, X[k] = X[0]
//     edge j: dx = |X[j+1] - X[j]|, dy likewise, L = max(dx, dy); it is walked from its smaller major coordinate (end points swapped when
//       that is its end: flip) with slope s = minor difference / L, and emits L + 1 points in its ORIGINAL direction: t = flip ? L - d : d,
//       major = t + start, minor = (int)(start + s t + .5).  L = 0: the single point (X[j], Y[j]); its 0 / 0 slope is never formed.
//     every consecutive pair of points (within an edge and across a junction) with u[j] != u[j-1] is a crossing when xi = (u[j] < u[j-1] ?
//       u[j] : u[j] - 1) sits on a pixel centre, (xi + .5) / 5 - .5 = x an integer in [0, w-1]; its row is yd = ceil(clamp((yi + .5) / 5
//       - .5, 0, h)) with yi = min(v[j], v[j-1]); its position is x h + yd in COLUMN-major order (yd = h: row 0 of the next column)
//     pixel (x, y) is set iff the number of crossings at positions <= x h + y is odd -- parity over the LINEAR position, so a column that
//       the polygon leaves through the bottom hands its odd count on to the next one
//   an instance is the OR of its polygons.
// The crossing test is integer here: (xi + .5) / 5 - .5 is an integer exactly when xi = 5 x + 2 (then the double quotient is exact; every
// other xi is at least .2 away from one), and ceil((yi + .5) / 5 - .5) = ceil((yi - 2) / 5) for the same reason.  The points themselves keep
// the double arithmetic, one rounding per operation (no contraction).
// Guard (not in pycocotools): a polygon with a non-finite coordinate (flag 1) or |5 c| > 5 * 32768 (flag 2) contributes nothing and its flags
// are OR-ed into the instance's status word; so L <= 2 * 163841 and every loop below is bounded by the sizes the caller passed.
//   abr_poly_rasterize     guard (a workgroup per instance) -> toggle planes of h w + 1 bits per polygon, zeroed -> edges: work items are
//                          (edge, step d) pairs, each compares point d with d - 1 and XORs one bit -> prefix parity along the plane, a
//                          workgroup per polygon, carried across words -> output (mask_out.h): each pixel ORs its instance's planes at x h + y
//   abr_poly_mask_targets  a workgroup per RoI: match the instance (mask_match.h), crop + resize the vertices in registers, the same edge
//                          walk into an LDS toggle grid per polygon, prefix parity, OR into an LDS accumulator, write [M,M] fp32
// Safety: offsets are clamped into the buffers as the RLE decoder does; every address written is derived from n, h, w, M and P_max.
#include <algorithm>

#include "common.h"
#include "mask_match.h"
#include "mask_out.h"

// every rounding below is part of the definition: one per operation, no fused multiply-add
#pragma clang fp contract(off)

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kEdgeThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kMaxM = 64;                                   // the LDS grid of abr_poly_mask_targets
constexpr int kMaxWords32 = (kMaxM * kMaxM + 1 + 31) / 32;  // 129

// ------------------------------------------------------------------------------------------------------------------ the edge walk
__device__ __forceinline__ int poly_guard(const float c) {
    if (!isfinite(c)) return 1;
    return fabs(5.0 * (double)c) > 5.0 * 32768.0 ? 2 : 0;
}

__device__ __forceinline__ int poly_up(const float c) {      // (int)(5 c + .5): truncation toward zero; 5 c is exact in double
    const double up = 5.0 * (double)c;
    return (int)(up + 0.5);
}

struct PolyEdge {
    int a0, b0;     // start after the swap: major, minor coordinate
    int L;
    bool xmajor, flip;
    double s;
};

__device__ __forceinline__ PolyEdge poly_edge(int xs, int ys, int xe, int ye) {
    PolyEdge e;
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    e.xmajor = dx >= dy;
    e.flip = (e.xmajor && xs > xe) || (!e.xmajor && ys > ye);
    if (e.flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    e.L = e.xmajor ? dx : dy;
    e.a0 = e.xmajor ? xs : ys;
    e.b0 = e.xmajor ? ys : xs;
    const int minor = e.xmajor ? ye - ys : xe - xs;
    e.s = e.L > 0 ? (double)minor / (double)e.L : 0.0;
    return e;
}

__device__ __forceinline__ void poly_point(const PolyEdge& e, const int d, int& u, int& v) {
    const int t = e.flip ? e.L - d : d;
    const int major = t + e.a0;
    const double st = e.s * (double)t;          // (plain operators: the pragma above keeps each its own rounding; the
    const double at = (double)e.b0 + st;        // __dmul_rn / __dadd_rn wrappers are compiled before it and may fuse)
    const int minor = e.L > 0 ? (int)(at + 0.5) : e.b0;
    u = e.xmajor ? major : minor;
    v = e.xmajor ? minor : major;
}

// the column-major position of the crossing between consecutive points (u0,v0) -> (u1,v1), or -1
__device__ __forceinline__ i64 poly_crossing(const int u0, const int v0, const int u1, const int v1, const int h, const int w) {
    if (u1 == u0) return -1;
    const int xi = u1 < u0 ? u1 : u1 - 1;
    if (xi < 0 || xi % 5 != 2) return -1;
    const int x = (xi - 2) / 5;
    if (x > w - 1) return -1;
    const int n = (v1 < v0 ? v1 : v0) - 2;
    int yd = n <= 0 ? 0 : (n + 4) / 5;
    if (yd > h) yd = h;
    return (i64)x * h + yd;
}

struct PolyRange { i64 lo, hi; };
__device__ __forceinline__ PolyRange poly_range(const i64* __restrict__ offsets, const i64 k, const i64 limit) {
    PolyRange r;
    r.lo = abr::clamp64(offsets[k], 0, limit);
    r.hi = abr::clamp64(offsets[k + 1], r.lo, limit);
    return r;
}

// ------------------------------------------------------------------------------------------------------------------ whole images
// flags[p] = guard flags of polygon p, status[i] = their OR over the instance's polygons
__global__ __launch_bounds__(kEdgeThreads) void poly_guard_kernel(const float* __restrict__ coords, const i64* __restrict__ poly_offsets,
                                                                 const i64* __restrict__ inst_offsets, i64 n_poly, i64 n_vert,
                                                                 int32_t* __restrict__ flags, int32_t* __restrict__ status) {
    const int i = blockIdx.x;
    const PolyRange pr = poly_range(inst_offsets, i, n_poly);
    int st = 0;
    for (i64 p = pr.lo; p < pr.hi; p++) {                                    // (workgroup-uniform)
        const PolyRange vr = poly_range(poly_offsets, p, n_vert);
        int f = 0;
        for (i64 j = vr.lo + threadIdx.x; j < vr.hi; j += kEdgeThreads) f |= poly_guard(coords[2 * j]) | poly_guard(coords[2 * j + 1]);
        const int f1 = __syncthreads_or(f & 1), f2 = __syncthreads_or(f & 2);
        const int all = (f1 ? 1 : 0) | (f2 ? 2 : 0);
        if (threadIdx.x == 0) flags[p] = all;       // (a polygon two instances claim gets the same value from both)
        st |= all;
    }
    if (threadIdx.x == 0) status[i] = st;
}

// grid (n_poly, splits): workgroup (p, s) walks edges s, s + splits, ... of polygon p
__global__ __launch_bounds__(kEdgeThreads) void poly_edges_kernel(const float* __restrict__ coords, const i64* __restrict__ poly_offsets, i64 n_poly,
                                                                 i64 n_vert, const int32_t* __restrict__ flags, int h, int w, i64 Cq,
                                                                 u64* __restrict__ planes) {
    const i64 p = blockIdx.x;
    if (flags[p]) return;
    const PolyRange vr = poly_range(poly_offsets, p, n_vert);
    const i64 k = vr.hi - vr.lo;
    const float* c = coords + 2 * vr.lo;
    u64* plane = planes + p * Cq;
    for (i64 j = blockIdx.y; j < k; j += gridDim.y) {
        const i64 jn = j + 1 < k ? j + 1 : 0;
        const int x0 = poly_up(c[2 * j]), y0 = poly_up(c[2 * j + 1]), x1 = poly_up(c[2 * jn]), y1 = poly_up(c[2 * jn + 1]);
        const PolyEdge e = poly_edge(x0, y0, x1, y1);
        for (int d = threadIdx.x + 1; d <= e.L; d += kEdgeThreads) {
            int ua, va, ub, vb;
            poly_point(e, d - 1, ua, va);
            poly_point(e, d, ub, vb);
            const i64 pos = poly_crossing(ua, va, ub, vb, h, w);              // pos <= h w: inside the plane's h w + 1 bits
            if (pos >= 0) atomicXor(&plane[pos >> 6], 1ull << (pos & 63));
        }
        if (threadIdx.x == 0 && j > 0) {                                      // the junction with the edge before
            const PolyEdge e0 = poly_edge(poly_up(c[2 * (j - 1)]), poly_up(c[2 * (j - 1) + 1]), x0, y0);
            int ua, va, ub, vb;
            poly_point(e0, e0.L, ua, va);
            poly_point(e, 0, ub, vb);
            const i64 pos = poly_crossing(ua, va, ub, vb, h, w);
            if (pos >= 0) atomicXor(&plane[pos >> 6], 1ull << (pos & 63));
        }
    }
}

__device__ __forceinline__ u64 prefix_xor64(u64 v) {
    v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;
    return v;
}

// toggles -> filled, in place: bit q of the plane becomes the parity of the toggles at positions <= q
__global__ __launch_bounds__(kScanThreads) void poly_parity_kernel(const int32_t* __restrict__ flags, i64 Cq, u64* __restrict__ planes) {
    __shared__ int sm[kScanThreads / 64];
    const i64 p = blockIdx.x;
    if (flags[p]) return;                                   // (its plane stays zero)
    u64* plane = planes + p * Cq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (i64 base = 0; base < Cq; base += kScanThreads) {
        const i64 q = base + threadIdx.x;
        const u64 f = q < Cq ? prefix_xor64(plane[q]) : 0ull;
        const u64 odd = __ballot((f >> 63) & 1ull);          // the words of this wave with an odd number of toggles
        const int before = __popcll(odd & ((1ull << lane) - 1ull)) & 1;
        __syncthreads();
        if (lane == 0) sm[wave] = __popcll(odd) & 1;
        __syncthreads();
        int in = carry, tot = carry;
#pragma unroll
        for (int i = 0; i < kScanThreads / 64; i++) {
            const int s = sm[i];
            if (i < wave) in ^= s;
            tot ^= s;
        }
        if (q < Cq) plane[q] = ((in ^ before) & 1) ? ~f : f;
        carry = tot;
    }
}

// the pixel predicate of the two outputs (mask_out.h): the OR of the instance's planes at the column-major position x h + y
struct PolyPixel {
    const u64* planes;
    const i64* inst_offsets;
    i64 n_poly, Cq;
    int h;
    PolyRange pr;
    __device__ __forceinline__ void instance(i64 k) { pr = poly_range(inst_offsets, k, n_poly); }
    __device__ __forceinline__ bool operator()(i64, int y, int x) const {
        const i64 pos = (i64)x * h + y;
        u64 any = 0;
        for (i64 p = pr.lo; p < pr.hi; p++) any |= planes[p * Cq + (pos >> 6)] >> (pos & 63);
        return (any & 1ull) != 0;
    }
};

__global__ __launch_bounds__(256) void poly_out_u8_kernel(const u64* __restrict__ planes, const i64* __restrict__ inst_offsets, i64 n_poly, i64 Cq, int h, int w,
                                                          i64 numel, uint8_t* __restrict__ out) {
    abr::mask_write_u8(PolyPixel{planes, inst_offsets, n_poly, Cq, h, {0, 0}}, numel, h, w, out);
}

__global__ __launch_bounds__(256) void poly_out_bits_kernel(const u64* __restrict__ planes, const i64* __restrict__ inst_offsets, i64 n_poly, i64 Cq, int h, int w,
                                                            int Wq, i64 n_words, u64* __restrict__ bits) {
    abr::mask_write_bits(PolyPixel{planes, inst_offsets, n_poly, Cq, h, {0, 0}}, n_words, h, w, Wq, bits);
}

// ------------------------------------------------------------------------------------------------------------------ M x M targets
// PolygonInstance.crop(box).resize((M, M)) of one coordinate: fl32(fl32(p - lo) * r), one rounding each
__device__ __forceinline__ float poly_project(const float p, const float lo, const float r) {
    const float moved = p - lo;
    return moved * r;
}

__device__ __forceinline__ unsigned prefix_xor32(unsigned v) {
    v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;
    return v;
}

// dims int32 [N,5]: instances (= ground-truth boxes), polygons, vertices, image height, image width
__global__ __launch_bounds__(kEdgeThreads) void poly_targets_kernel(const float* const* __restrict__ coord_ptrs, const i64* const* __restrict__ poff_ptrs,
                                                                   const i64* const* __restrict__ ioff_ptrs, const int32_t* __restrict__ dims,
                                                                   const float* const* __restrict__ gt_ptrs, const float* __restrict__ rois,
                                                                   const int64_t* __restrict__ pos_rows, int K, int N, int M, float* __restrict__ out) {
    __shared__ unsigned tog[kMaxWords32], acc[kMaxWords32], par[kMaxWords32];
    __shared__ float sf[4];
    __shared__ int s_inst;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int64_t row = pos_rows[p];
    float* o = out + (int64_t)p * M * M;
    int img = -1;
    if (row >= 0 && row < K) img = (int)rois[row * 5];
    if (img < 0 || img >= N || dims[img * 5] <= 0) {   // padding row
        for (int i = tid; i < M * M; i += kEdgeThreads) o[i] = 0.f;
        return;
    }
    const int G = dims[img * 5], n_poly = dims[img * 5 + 1], n_vert = dims[img * 5 + 2], H = dims[img * 5 + 3], W = dims[img * 5 + 4];
    if (tid == 0) {
        const float4 b = make_float4(rois[row * 5 + 1], rois[row * 5 + 2], rois[row * 5 + 3], rois[row * 5 + 4]);
        s_inst = abr::mask_match_gt(reinterpret_cast<const float4*>(gt_ptrs[img]), G, b);
        // PolygonInstance.crop (segmentation_mask.py:246-263): the box as Python floats, clamped against the image size
        double xmin = b.x, ymin = b.y, xmax = b.z, ymax = b.w;
        xmin = fmin(fmax(xmin, 0.0), (double)(W - 1));
        ymin = fmin(fmax(ymin, 0.0), (double)(H - 1));
        xmax = fmin(fmax(xmax, 0.0), (double)W);
        ymax = fmin(fmax(ymax, 0.0), (double)H);
        xmax = fmax(xmax, xmin + 1.0);
        ymax = fmax(ymax, ymin + 1.0);
        // .resize((M, M)) (:281): float(M) / float(w) in double; the fp32 tensor multiplies by it rounded to fp32
        sf[0] = (float)xmin;
        sf[1] = (float)ymin;
        sf[2] = (float)((double)M / (xmax - xmin));
        sf[3] = (float)((double)M / (ymax - ymin));
    }
    const int nW = (M * M + 1 + 31) / 32;
    for (int i = tid; i < nW; i += kEdgeThreads) acc[i] = 0u;
    __syncthreads();
    const float lox = sf[0], loy = sf[1], rx = sf[2], ry = sf[3];
    const float* coords = coord_ptrs[img];
    const i64* poff = poff_ptrs[img];
    const PolyRange pr = poly_range(ioff_ptrs[img], s_inst, n_poly);
    for (i64 q = pr.lo; q < pr.hi; q++) {                                    // (workgroup-uniform)
        const PolyRange vr = poly_range(poff, q, n_vert);
        const i64 k = vr.hi - vr.lo;
        const float* c = coords + 2 * vr.lo;
        int f = 0;
        for (i64 j = tid; j < k; j += kEdgeThreads) f |= poly_guard(poly_project(c[2 * j], lox, rx)) | poly_guard(poly_project(c[2 * j + 1], loy, ry));
        for (int i = tid; i < nW; i += kEdgeThreads) tog[i] = 0u;
        if (__syncthreads_or(f)) continue;                                   // guarded: contributes nothing
        for (i64 j = 0; j < k; j++) {
            const i64 jn = j + 1 < k ? j + 1 : 0;
            const int x0 = poly_up(poly_project(c[2 * j], lox, rx)), y0 = poly_up(poly_project(c[2 * j + 1], loy, ry));
            const int x1 = poly_up(poly_project(c[2 * jn], lox, rx)), y1 = poly_up(poly_project(c[2 * jn + 1], loy, ry));
            const PolyEdge e = poly_edge(x0, y0, x1, y1);
            for (int d = tid + 1; d <= e.L; d += kEdgeThreads) {
                int ua, va, ub, vb;
                poly_point(e, d - 1, ua, va);
                poly_point(e, d, ub, vb);
                const i64 pos = poly_crossing(ua, va, ub, vb, M, M);          // pos <= M M < 32 nW
                if (pos >= 0) atomicXor(&tog[pos >> 5], 1u << (pos & 31));
            }
            if (tid == 0 && j > 0) {
                const PolyEdge e0 = poly_edge(poly_up(poly_project(c[2 * (j - 1)], lox, rx)), poly_up(poly_project(c[2 * (j - 1) + 1], loy, ry)), x0, y0);
                int ua, va, ub, vb;
                poly_point(e0, e0.L, ua, va);
                poly_point(e, 0, ub, vb);
                const i64 pos = poly_crossing(ua, va, ub, vb, M, M);
                if (pos >= 0) atomicXor(&tog[pos >> 5], 1u << (pos & 31));
            }
        }
        __syncthreads();
        for (int i = tid; i < nW; i += kEdgeThreads) {
            const unsigned v = prefix_xor32(tog[i]);
            tog[i] = v;
            par[i] = v >> 31;
        }
        __syncthreads();
        for (int i = tid; i < nW; i += kEdgeThreads) {
            unsigned in = 0u;
            for (int b = 0; b < i; b++) in ^= par[b];
            acc[i] |= in ? ~tog[i] : tog[i];
        }
        __syncthreads();                                                     // tog is zeroed again by the next polygon
    }
    __syncthreads();
    for (int i = tid; i < M * M; i += kEdgeThreads) {
        const int oy = i / M, ox = i - oy * M;
        const int pos = ox * M + oy;
        o[i] = (float)((acc[pos >> 5] >> (pos & 31)) & 1u);
    }
}

bool image_ok(int h, int w) { return h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31) - 64; }
int64_t plane_words(int h, int w) { return ((int64_t)h * w + 1 + 63) / 64; }
int64_t flag_bytes(int64_t n_poly) { return (n_poly * 4 + 7) / 8 * 8; }

}  // namespace

extern "C" int64_t abr_poly_rasterize_workspace_bytes(int64_t n_poly, int h, int w) {
    if (n_poly < 0 || !image_ok(h, w)) return -1;
    return flag_bytes(n_poly) + n_poly * plane_words(h, w) * 8;
}

extern "C" int abr_poly_rasterize(const float* coords, const int64_t* poly_offsets, const int64_t* inst_offsets, int n, int64_t n_poly, int64_t n_vert,
                                  int h, int w, uint8_t* masks, uint64_t* bits, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    ABR_REQUIRE(n >= 0 && n_poly >= 0 && n_poly < ((int64_t)1 << 31) && n_vert >= 0 && n_vert < ((int64_t)1 << 40) && image_ok(h, w),
                "poly_rasterize: bad args (n, n_poly, n_vert >= 0, n_poly < 2^31, 0 < h * w < 2^31 - 64)");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(inst_offsets && status && (masks || bits), "poly_rasterize: null pointer (inst_offsets, status and at least one of masks / bits)");
    ABR_REQUIRE(n_poly == 0 || poly_offsets, "poly_rasterize: null poly_offsets");
    ABR_REQUIRE(n_vert == 0 || coords, "poly_rasterize: null coords");
    ABR_REQUIRE((reinterpret_cast<uintptr_t>(masks) & 3) == 0 && (reinterpret_cast<uintptr_t>(bits) & 7) == 0, "poly_rasterize: masks must be 4-byte aligned, bits 8-byte aligned");
    const int64_t need = abr_poly_rasterize_workspace_bytes(n_poly, h, w);
    if (workspace_bytes < need || (need > 0 && !workspace) || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
        abr::set_error("poly_rasterize: workspace of %lld bytes, abr_poly_rasterize_workspace_bytes asks for %lld (8-byte aligned)", (long long)workspace_bytes,
                       (long long)need);
        return ABR_E_WORKSPACE;
    }
    hipStream_t st = abr::as_stream(stream);
    int32_t* flags = static_cast<int32_t*>(workspace);
    u64* planes = reinterpret_cast<u64*>(static_cast<char*>(workspace) + flag_bytes(n_poly));
    const i64* poff = reinterpret_cast<const i64*>(poly_offsets);
    const i64* ioff = reinterpret_cast<const i64*>(inst_offsets);
    const int64_t Cq = plane_words(h, w);
    if (n_poly > 0) {
        ABR_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)need, st) == hipSuccess, "poly_rasterize: hipMemsetAsync failed");
    }
    poly_guard_kernel<<<n, kEdgeThreads, 0, st>>>(coords, poff, ioff, n_poly, n_vert, flags, status);
    ABR_CHECK_LAUNCH("poly_rasterize (guard)");
    if (n_poly > 0) {
        const unsigned splits = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, 2048 / n_poly));
        poly_edges_kernel<<<dim3((unsigned)n_poly, splits), kEdgeThreads, 0, st>>>(coords, poff, n_poly, n_vert, flags, h, w, Cq, planes);
        ABR_CHECK_LAUNCH("poly_rasterize (edges)");
        poly_parity_kernel<<<(unsigned)n_poly, kScanThreads, 0, st>>>(flags, Cq, planes);
        ABR_CHECK_LAUNCH("poly_rasterize (parity)");
    }
    if (masks) {
        const int64_t numel = (int64_t)n * h * w;
        poly_out_u8_kernel<<<abr::quad_grid(numel), 256, 0, st>>>(planes, ioff, n_poly, Cq, h, w, numel, masks);
        ABR_CHECK_LAUNCH("poly_rasterize (masks)");
    }
    if (bits) {
        const int Wq = (w + 63) / 64;
        const int64_t n_words = (int64_t)n * h * Wq;
        poly_out_bits_kernel<<<abr::wave_grid(n_words), 256, 0, st>>>(planes, ioff, n_poly, Cq, h, w, Wq, n_words, reinterpret_cast<u64*>(bits));
        ABR_CHECK_LAUNCH("poly_rasterize (bits)");
    }
    return ABR_OK;
}

extern "C" int abr_poly_mask_targets(const float* const* coord_ptrs, const int64_t* const* poly_offset_ptrs, const int64_t* const* inst_offset_ptrs,
                                     const int32_t* dims, const float* const* gt_ptrs, const float* rois, const int64_t* pos_rows, int P_max, int K, int N,
                                     int M, float* out, void* stream) {
    ABR_REQUIRE(P_max >= 0 && K >= 0 && N > 0 && M > 0 && M <= kMaxM, "poly_mask_targets: bad args (0 < M <= 64)");
    if (P_max == 0) return ABR_OK;
    ABR_REQUIRE(coord_ptrs && poly_offset_ptrs && inst_offset_ptrs && dims && gt_ptrs && rois && pos_rows && out, "poly_mask_targets: null pointer");
    poly_targets_kernel<<<P_max, kEdgeThreads, 0, abr::as_stream(stream)>>>(coord_ptrs, reinterpret_cast<const i64* const*>(poly_offset_ptrs),
                                                                           reinterpret_cast<const i64* const*>(inst_offset_ptrs), dims, gt_ptrs, rois, pos_rows,
                                                                           K, N, M, out);
    ABR_CHECK_LAUNCH("poly_mask_targets");
    return ABR_OK;
}
