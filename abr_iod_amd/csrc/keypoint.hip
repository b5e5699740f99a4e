// Keypoint head (MODEL.KEYPOINT_ON, KeypointRCNNFeatureExtractor + KeypointRCNNPredictor) -- the kernels around its contractions, which run
// on the conv planner:
//   targets: positives with a visible keypoint, heat-map indices     keypoint_head/loss.py:39-143, structures/keypoint.py:154-188
//   ConvTranspose2d(C, K, 4, 2, 1) as GEMM + fold, and the adjoint   keypoint_head/roi_keypoint_predictors.py:8-33
//   bilinear 2x upsampling of the low-resolution maps (eval)         roi_keypoint_predictors.py:29-32
//   fused upsampling + spatial softmax cross-entropy + gradient      keypoint_head/loss.py:145-169
//   heat maps -> keypoints (bicubic resize to the RoI, argmax)       keypoint_head/inference.py:40-94
// The low-resolution maps are PLANAR [P,Kp,2h,2w], Kp = K rounded up to a multiple of 4: the loss and the decode own one contiguous plane per
// (RoI, keypoint).  fp32 arithmetic, no floating-point atomics: every sum has a fixed order, so two runs agree bit for bit.
#include <algorithm>

#include "common.h"
#include "mask_match.h"

namespace {

constexpr int kKpMaxPlane = 4096;     // floats of one plane staged in LDS (16 KB): kp_loss's H*W and kp_decode's Hm*Wm

// ------------------------------------------------------------------------------------------------
// targets (one workgroup for the whole batch: the sampled set is a few thousand rows)
// ------------------------------------------------------------------------------------------------
// keypoints_to_heat_map's index along one axis: floor((v - lo) * scale), the v == hi rule, -1 where it leaves [0, M) (inf / NaN too).
// scale = heatmap_size / (hi - lo) with a Python number on the left is torch's reciprocal() * heatmap_size: two roundings, not one division
__device__ __forceinline__ int kp_heat_index(const float v, const float lo, const float hi, const int M) {
#pragma clang fp contract(off)      // (one rounding per operation, as torch; this function alone: the other kernels may contract)
    const float scale = (1.f / (hi - lo)) * (float)M;
    const float f = floorf((v - lo) * scale);
    int i = (f >= 0.f && f < (float)M) ? (int)f : -1;
    if (v == hi) i = M - 1;
    return i;
}

__global__ __launch_bounds__(1024) void kp_select_targets_kernel(const float* __restrict__ rois, const int64_t* __restrict__ labels, int R,
                                                                 const float* const* __restrict__ gt_ptrs, const float* const* __restrict__ kp_ptrs,
                                                                 const int32_t* __restrict__ n_gt, int N, int K, int M, int P_max,
                                                                 int64_t* __restrict__ pos_rows, int64_t* __restrict__ inv, int32_t* __restrict__ n_pos,
                                                                 int64_t* __restrict__ tgt, uint8_t* __restrict__ valid, int32_t* __restrict__ n_valid) {
    __shared__ int s_wave[16];
    __shared__ int s_valid;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_valid = 0;
    int base = 0, my_valid = 0;
    for (int start = 0; start < R; start += 1024) {
        const int i = start + tid;
        bool flag = false;
        int gi = 0;
        const float* kp = nullptr;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < R && labels[i] > 0) {
            const int img = (int)rois[(int64_t)i * 5];
            if (img >= 0 && img < N && n_gt[img] > 0) {
                b = make_float4(rois[(int64_t)i * 5 + 1], rois[(int64_t)i * 5 + 2], rois[(int64_t)i * 5 + 3], rois[(int64_t)i * 5 + 4]);
                const float4* gt = reinterpret_cast<const float4*>(gt_ptrs[img]);
                gi = abr::mask_match_gt(gt, n_gt[img], b);       // first maximum IoU (mask_match.h)
                const float4 g = gt[gi];
                kp = kp_ptrs[img] + (int64_t)gi * K * 3;
                for (int k = 0; k < K; k++) {                    // _within_box (inclusive) & visible, loss.py:98-102
                    const float x = kp[k * 3], y = kp[k * 3 + 1], v = kp[k * 3 + 2];
                    flag = flag || (v > 0.f && x >= g.x && x <= g.z && y >= g.y && y <= g.w);
                }
            }
        }
        const unsigned long long bal = __ballot(flag);
        const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int c = s_wave[w];
            off += w < wv ? c : 0;
            tot += c;
        }
        if (i < R) {
            const int p = base + off + prefix;
            const bool take = flag && p < P_max;
            if (take) {
                pos_rows[p] = i;
                for (int k = 0; k < K; k++) {
                    const int xi = kp_heat_index(kp[k * 3], b.x, b.z, M), yi = kp_heat_index(kp[k * 3 + 1], b.y, b.w, M);
                    const bool ok = xi >= 0 && yi >= 0 && xi < M && yi < M && kp[k * 3 + 2] > 0.f;
                    tgt[(int64_t)p * K + k] = ok ? (int64_t)yi * M + xi : 0;
                    valid[(int64_t)p * K + k] = ok ? 1 : 0;
                    my_valid += ok ? 1 : 0;
                }
            }
            inv[i] = take ? p : -1;
        }
        base += tot;
    }
    const int n = min(base, P_max);
    for (int p = n + tid; p < P_max; p += 1024) pos_rows[p] = -1;
    for (int64_t e = (int64_t)n * K + tid; e < (int64_t)P_max * K; e += 1024) {
        tgt[e] = 0;
        valid[e] = 0;
    }
    if (my_valid) atomicAdd(&s_valid, my_valid);      // (integers: any order gives the same sum)
    __syncthreads();
    if (tid == 0) {
        *n_pos = n;
        *n_valid = s_valid;
    }
}

// ------------------------------------------------------------------------------------------------
// ConvTranspose2d(k=4, s=2, p=1) as GEMM + fold: y [P,h,w,(ky,kx,k)] -> out [P,Kp,2h,2w]
// output row oy takes the taps ky = (oy + 1) & 1 and ky + 2 from input rows iy = (oy + 1 - ky) / 2 (at most two inside the map)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kp_fold_kernel(const float4* __restrict__ y, const float* __restrict__ bias, int64_t total, int h, int w,
                                                      int K, int Kp, float* __restrict__ out) {
    const int H = 2 * h, W = 2 * w, k4n = Kp >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % W);
        int64_t t = i / W;
        const int oy = (int)(t % H);
        t /= H;
        const int k4 = (int)(t % k4n);
        const int64_t p = t / k4n;
        float4 a;
        a.x = 4 * k4 < K ? bias[4 * k4] : 0.f;
        a.y = 4 * k4 + 1 < K ? bias[4 * k4 + 1] : 0.f;
        a.z = 4 * k4 + 2 < K ? bias[4 * k4 + 2] : 0.f;
        a.w = 4 * k4 + 3 < K ? bias[4 * k4 + 3] : 0.f;
        for (int ky = (oy + 1) & 1; ky < 4; ky += 2) {
            const int iy = (oy + 1 - ky) >> 1;
            if (iy < 0 || iy >= h) continue;
            for (int kx = (ox + 1) & 1; kx < 4; kx += 2) {
                const int ix = (ox + 1 - kx) >> 1;
                if (ix < 0 || ix >= w) continue;
                const float4 v = y[(((p * h + iy) * w + ix) * 16 + ky * 4 + kx) * k4n + k4];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        }
        float* o = out + ((p * Kp + 4 * k4) * H + oy) * W + ox;
        const int64_t plane = (int64_t)H * W;
        o[0] = 4 * k4 < K ? a.x : 0.f;
        o[plane] = 4 * k4 + 1 < K ? a.y : 0.f;
        o[2 * plane] = 4 * k4 + 2 < K ? a.z : 0.f;
        o[3 * plane] = 4 * k4 + 3 < K ? a.w : 0.f;
    }
}

// the exact adjoint: gy [P,h,w,(ky,kx,k)] = g [p,k,2iy-1+ky,2ix-1+kx], zero outside the map and for k >= K
__global__ __launch_bounds__(256) void kp_unfold_kernel(const float* __restrict__ g, int64_t total4, int h, int w, int K, int Kp,
                                                        float4* __restrict__ gy) {
    const int H = 2 * h, W = 2 * w, k4n = Kp >> 2;
    const int64_t plane = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int k4 = (int)(i % k4n);
        int64_t t = i / k4n;
        const int tap = (int)(t & 15);
        t >>= 4;
        const int ix = (int)(t % w);
        t /= w;
        const int iy = (int)(t % h);
        const int64_t p = t / h;
        const int oy = 2 * iy - 1 + (tap >> 2), ox = 2 * ix - 1 + (tap & 3);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
            const float* s = g + ((p * Kp + 4 * k4) * H + oy) * W + ox;
            if (4 * k4 < K) v.x = s[0];
            if (4 * k4 + 1 < K) v.y = s[plane];
            if (4 * k4 + 2 < K) v.z = s[2 * plane];
            if (4 * k4 + 3 < K) v.w = s[3 * plane];
        }
        gy[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// bilinear 2x, align_corners=False: source coordinate (d + 0.5) / 2 - 0.5 clamped at 0, the far tap replicated at the edge
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void up2_tap(const int d, const int n, int& i0, int& i1, float& l) {
    const float s = fmaxf(((float)d + 0.5f) * 0.5f - 0.5f, 0.f);
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    l = s - (float)i0;
}

// the upsampled value at (oy, ox) of an H x W plane
__device__ __forceinline__ float up2_at(const float* __restrict__ pl, const int H, const int W, const int oy, const int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    up2_tap(oy, H, y0, y1, ly);
    up2_tap(ox, W, x0, x1, lx);
    const float top = (1.f - lx) * pl[y0 * W + x0] + lx * pl[y0 * W + x1];
    const float bot = (1.f - lx) * pl[y1 * W + x0] + lx * pl[y1 * W + x1];
    return (1.f - ly) * top + ly * bot;
}

__global__ __launch_bounds__(256) void kp_upsample2x_kernel(const float* __restrict__ x, int64_t total, int H, int W, int K, int Kp,
                                                            float* __restrict__ out) {
    const int H2 = 2 * H, W2 = 2 * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % W2);
        int64_t t = i / W2;
        const int oy = (int)(t % H2);
        t /= H2;
        const int k = (int)(t % K);
        const int64_t p = t / K;
        out[i] = up2_at(x + (p * Kp + k) * (int64_t)H * W, H, W, oy, ox);
    }
}

// ------------------------------------------------------------------------------------------------
// loss: one workgroup per (RoI, channel) row.  The H x W plane is staged in LDS; the 4 H W upsampled logits are formed on the fly for the
// maximum, for the exp-sum and again for the gradient, which every low-resolution pixel GATHERS from the at most 4 x 4 upsampled pixels whose
// stencil holds it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_max4(float v, float* sm) {
    v = abr::wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// weight of low-resolution index i in the stencil of upsampled index o
__device__ __forceinline__ float up2_weight(const int o, const int n, const int i) {
    int i0, i1;
    float l;
    up2_tap(o, n, i0, i1, l);
    return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

__global__ __launch_bounds__(256) void kp_loss_kernel(const float* __restrict__ x, int H, int W, int K, int Kp, const int64_t* __restrict__ tgt,
                                                      const uint8_t* __restrict__ valid, const int32_t* __restrict__ n_valid, float gscale,
                                                      float* __restrict__ loss_out, float* __restrict__ grad, float* __restrict__ row_sum,
                                                      const abr::DetWs ws) {
    __shared__ float s_pl[kKpMaxPlane];
    __shared__ float sm[4];
    const int row = blockIdx.x, p = row / Kp, k = row - p * Kp;
    const int HW = H * W, H2 = 2 * H, W2 = 2 * W, n_up = 4 * HW;
    const int nv = *n_valid;
    int64_t t = -1;
    if (k < K && nv > 0 && valid[(int64_t)p * K + k]) t = tgt[(int64_t)p * K + k];
    const bool live = t >= 0 && t < n_up;      // (uniform over the workgroup)
    float ce = 0.f;
    if (live) {
        const float* pl = x + (int64_t)row * HW;
        for (int i = threadIdx.x; i < HW; i += 256) s_pl[i] = pl[i];
        __syncthreads();
        float m = -INFINITY;
        for (int j = threadIdx.x; j < n_up; j += 256) m = fmaxf(m, up2_at(s_pl, H, W, j / W2, j % W2));
        m = block_max4(m, sm);
        float s = 0.f;
        for (int j = threadIdx.x; j < n_up; j += 256) s += expf(up2_at(s_pl, H, W, j / W2, j % W2) - m);
        s = abr::block_sum<4>(s, sm);
        const int ty = (int)(t / W2), tx = (int)(t - (int64_t)ty * W2);
        ce = logf(s) + m - up2_at(s_pl, H, W, ty, tx);
        if (grad) {
            const float inv_s = 1.f / s, sc = gscale / (float)nv;
            float acc = 0.f;
            for (int i = threadIdx.x; i < HW; i += 256) {
                const int iy = i / W, ix = i - iy * W;
                float g = 0.f;
                for (int oy = max(2 * iy - 1, 0); oy <= min(2 * iy + 2, H2 - 1); oy++) {
                    const float wy = up2_weight(oy, H, iy);
                    for (int ox = max(2 * ix - 1, 0); ox <= min(2 * ix + 2, W2 - 1); ox++) {
                        const float wx = up2_weight(ox, W, ix);
                        const float sm_v = expf(up2_at(s_pl, H, W, oy, ox) - m) * inv_s;
                        g += wy * wx * (sm_v - ((oy == ty && ox == tx) ? 1.f : 0.f));
                    }
                }
                g *= sc;
                grad[(int64_t)row * HW + i] = g;
                acc += g;
            }
            acc = abr::block_sum<4>(acc, sm);
            if (threadIdx.x == 0 && row_sum) row_sum[row] = acc;
        }
    } else if (grad) {
        for (int i = threadIdx.x; i < HW; i += 256) grad[(int64_t)row * HW + i] = 0.f;
        if (threadIdx.x == 0 && row_sum) row_sum[row] = 0.f;
    }
    const float in[1] = {ce};
    float tot[1];
    if (abr::det_sum_last<1>(in, ws, tot) && threadIdx.x == 0) *loss_out = nv > 0 ? tot[0] / (float)nv : 0.f;
}

// ------------------------------------------------------------------------------------------------
// decode: one workgroup per (detection, keypoint).  The map is resized to ceil(max(w, 1)) x ceil(max(h, 1)) with the bicubic rule (Keys'
// kernel, a = -0.75, source coordinate (d + 0.5) src / dst - 0.5, replicated borders, no antialiasing) and the first maximum in row-major order
// is taken: among equal values the LOWEST index wins, through the per-thread scan, the wave shuffle and the cross-wave step alike.
// A NaN value never wins a comparison; a map of NaNs alone gives index 0.
// ------------------------------------------------------------------------------------------------
constexpr int kKpMaxGrid = 8192;      // the resized grid's side is clamped here (a non-finite or absurd box must not spin for ever)

__device__ __forceinline__ void cubic_taps(const int d, const float scale, const int n, int (&idx)[4], float (&c)[4]) {
    const float A = -0.75f;
    const float s = ((float)d + 0.5f) * scale - 0.5f;
    const float fl = floorf(s);
    const float f = s - fl;
    const int i = (int)fl;
    c[0] = ((A * (f + 1.f) - 5.f * A) * (f + 1.f) + 8.f * A) * (f + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
    c[2] = ((A + 2.f) * (1.f - f) - (A + 3.f)) * (1.f - f) * (1.f - f) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
#pragma unroll
    for (int j = 0; j < 4; j++) idx[j] = min(max(i - 1 + j, 0), n - 1);
}

__device__ __forceinline__ float cubic_at(const float* __restrict__ pl, const int Hm, const int Wm, const int y, const int x, const float sy,
                                          const float sx) {
    int iy[4], ix[4];
    float cy[4], cx[4];
    cubic_taps(y, sy, Hm, iy, cy);
    cubic_taps(x, sx, Wm, ix, cx);
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const float* r = pl + iy[a] * Wm;
        v += cy[a] * (cx[0] * r[ix[0]] + cx[1] * r[ix[1]] + cx[2] * r[ix[2]] + cx[3] * r[ix[3]]);
    }
    return v;
}

__device__ __forceinline__ int grid_side(const float extent) {     // ceil(max(extent, 1)) as an int in [1, kKpMaxGrid]
    const float c = ceilf(fmaxf(extent, 1.f));
    return c < (float)kKpMaxGrid ? (int)c : kKpMaxGrid;
}

// inference.py:73-90 in numpy's types: (index + 0.5) * correction + offset in float64 with a rounding after each operation, stored as float32
__device__ __forceinline__ float kp_coord(const int index, const float correction, const float offset) {
#pragma clang fp contract(off)
    const double prod = ((double)index + 0.5) * (double)correction;
    return (float)(prod + (double)offset);
}

// (value, index) pairs: does b beat a?
__device__ __forceinline__ bool kp_beats(const float bv, const int bi, const float av, const int ai) { return bv > av || (bv == av && bi < ai); }

__global__ __launch_bounds__(256) void kp_decode_kernel(const float* __restrict__ maps, int64_t map_stride_d, int64_t map_stride_k,
                                                        const float* __restrict__ boxes, int K, int Hm, int Wm, float* __restrict__ xy,
                                                        float* __restrict__ logit) {
    __shared__ float s_pl[kKpMaxPlane];
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int d = blockIdx.x / K, k = blockIdx.x - d * K;
    const float* pl = maps + d * map_stride_d + k * map_stride_k;
    for (int i = threadIdx.x; i < Hm * Wm; i += 256) s_pl[i] = pl[i];
    __syncthreads();
    const float x1 = boxes[d * 4], y1 = boxes[d * 4 + 1], x2 = boxes[d * 4 + 2], y2 = boxes[d * 4 + 3];
    const float bw = fmaxf(x2 - x1, 1.f), bh = fmaxf(y2 - y1, 1.f);
    const int gw = grid_side(x2 - x1), gh = grid_side(y2 - y1);
    const float sx = (float)Wm / (float)gw, sy = (float)Hm / (float)gh;
    const int total = gw * gh;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int yy = i / gw;
        const float v = cubic_at(s_pl, Hm, Wm, yy, i - yy * gw, sy, sx);
        if (kp_beats(v, i, best, bi)) { best = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (kp_beats(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (kp_beats(s_v[w], s_i[w], best, bi)) { best = s_v[w]; bi = s_i[w]; }
        if (bi == 0x7fffffff) bi = 0;      // nothing compared greater than -inf: a map of -inf or NaN
        const int yi = bi / gw, xi = bi - yi * gw;
        // the correction is a float32 quotient (kp_coord)
        const float wc = bw / (float)gw, hc = bh / (float)gh;
        float* o = xy + (int64_t)blockIdx.x * 3;
        o[0] = kp_coord(xi, wc, x1);
        o[1] = kp_coord(yi, hc, y1);
        o[2] = 1.f;
        logit[blockIdx.x] = cubic_at(s_pl, Hm, Wm, yi, xi, sy, sx);
    }
}

unsigned grid_for(int64_t work, unsigned cap = 4096u) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, cap)); }

}  // namespace

extern "C" int abr_kp_select_targets(const float* rois, const int64_t* labels, int R, const float* const* gt_ptrs, const float* const* kp_ptrs,
                                     const int32_t* n_gt, int N, int K, int M, int P_max, int64_t* pos_rows, int64_t* inv, int32_t* n_pos,
                                     int64_t* tgt, uint8_t* valid, int32_t* n_valid, void* stream) {
    ABR_REQUIRE(R >= 0 && N > 0 && K > 0 && M > 0 && M <= 32768 && P_max >= 0 && n_pos && n_valid, "kp_select_targets: bad args");
    ABR_REQUIRE((R == 0 || (rois && labels && inv)) && gt_ptrs && kp_ptrs && n_gt && (P_max == 0 || (pos_rows && tgt && valid)),
                "kp_select_targets: null pointer");
    kp_select_targets_kernel<<<1, 1024, 0, abr::as_stream(stream)>>>(rois, labels, R, gt_ptrs, kp_ptrs, n_gt, N, K, M, P_max, pos_rows, inv, n_pos,
                                                                    tgt, valid, n_valid);
    ABR_CHECK_LAUNCH("kp_select_targets");
    return ABR_OK;
}

extern "C" int abr_kp_deconv_fold(const float* y, const float* bias, int P, int h, int w, int K, float* out, void* stream) {
    ABR_REQUIRE(P >= 0 && h > 0 && w > 0 && K > 0 && h <= 16384 && w <= 16384, "kp_deconv_fold: bad args");
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(y && bias && out, "kp_deconv_fold: null pointer");
    const int Kp = (K + 3) / 4 * 4;
    const int64_t total = (int64_t)P * (Kp / 4) * 4 * h * w;
    kp_fold_kernel<<<grid_for(total), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(y), bias, total, h, w, K, Kp, out);
    ABR_CHECK_LAUNCH("kp_deconv_fold");
    return ABR_OK;
}

extern "C" int abr_kp_deconv_unfold(const float* g, int P, int h, int w, int K, float* gy, void* stream) {
    ABR_REQUIRE(P >= 0 && h > 0 && w > 0 && K > 0 && h <= 16384 && w <= 16384, "kp_deconv_unfold: bad args");
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(g && gy, "kp_deconv_unfold: null pointer");
    const int Kp = (K + 3) / 4 * 4;
    const int64_t total4 = (int64_t)P * h * w * 16 * (Kp / 4);
    kp_unfold_kernel<<<grid_for(total4), 256, 0, abr::as_stream(stream)>>>(g, total4, h, w, K, Kp, reinterpret_cast<float4*>(gy));
    ABR_CHECK_LAUNCH("kp_deconv_unfold");
    return ABR_OK;
}

extern "C" int abr_kp_upsample2x(const float* x, int P, int K, int H, int W, float* out, void* stream) {
    ABR_REQUIRE(P >= 0 && K > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "kp_upsample2x: bad args");
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(x && out, "kp_upsample2x: null pointer");
    const int64_t total = (int64_t)P * K * 4 * H * W;
    kp_upsample2x_kernel<<<grid_for(total), 256, 0, abr::as_stream(stream)>>>(x, total, H, W, K, (K + 3) / 4 * 4, out);
    ABR_CHECK_LAUNCH("kp_upsample2x");
    return ABR_OK;
}

extern "C" int abr_kp_loss_max_plane(void) { return kKpMaxPlane; }

extern "C" int abr_kp_loss(const float* x, int P, int K, int H, int W, const int64_t* tgt, const uint8_t* valid, const int32_t* n_valid,
                           float gscale, float* loss_out, float* grad, float* row_sum, void* stream) {
    ABR_REQUIRE(P >= 0 && K > 0 && H > 0 && W > 0 && loss_out && n_valid, "kp_loss: bad args");
    ABR_REQUIRE((int64_t)H * W <= kKpMaxPlane, "kp_loss: a %d x %d plane does not fit the %d floats staged in LDS", H, W, kKpMaxPlane);
    hipStream_t st = abr::as_stream(stream);
    if (hipMemsetAsync(loss_out, 0, sizeof(float), st) != hipSuccess) {
        abr::set_error("kp_loss: hipMemsetAsync failed");
        return ABR_E_LAUNCH;
    }
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(x && tgt && valid, "kp_loss: null pointer");
    const int Kp = (K + 3) / 4 * 4;
    const int64_t rows = (int64_t)P * Kp;
    ABR_REQUIRE(rows <= 65536, "kp_loss: more than 65536 (RoI, channel) rows");
    const abr::DetWs ws = abr::det_ws(st, (size_t)rows);
    ABR_REQUIRE(ws.part, "kp_loss: no device memory for the per-row losses");
    kp_loss_kernel<<<(unsigned)rows, 256, 0, st>>>(x, H, W, K, Kp, tgt, valid, n_valid, gscale, loss_out, grad, row_sum, ws);
    ABR_CHECK_LAUNCH("kp_loss");
    return ABR_OK;
}

extern "C" int abr_kp_decode(const float* maps, int64_t stride_d, int64_t stride_k, const float* boxes, int D, int K, int Hm, int Wm, float* xy,
                             float* logit, void* stream) {
    ABR_REQUIRE(D >= 0 && K > 0 && Hm > 0 && Wm > 0 && stride_k >= (int64_t)Hm * Wm && stride_d >= stride_k, "kp_decode: bad args");
    ABR_REQUIRE((int64_t)Hm * Wm <= kKpMaxPlane, "kp_decode: a %d x %d map does not fit the %d floats staged in LDS", Hm, Wm, kKpMaxPlane);
    if (D == 0) return ABR_OK;
    ABR_REQUIRE(maps && boxes && xy && logit, "kp_decode: null pointer");
    ABR_REQUIRE((int64_t)D * K <= 0x7fffffff, "kp_decode: too many (detection, keypoint) pairs");
    kp_decode_kernel<<<(unsigned)(D * K), 256, 0, abr::as_stream(stream)>>>(maps, stride_d, stride_k, boxes, K, Hm, Wm, xy, logit);
    ABR_CHECK_LAUNCH("kp_decode");
    return ABR_OK;
}
