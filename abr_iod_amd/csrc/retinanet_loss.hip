// RetinaNet's training loss over a feature pyramid: the anchors' labelled targets, both losses, and their gradient where the convs' backward
// reads it.
//
// Reference: maskrcnn_benchmark/modeling/rpn/retinanet/loss.py over rpn/loss.py:66-102 and rpn/utils.py:10-45.  Per image a Matcher with
// low-quality matches, the matched ground truth's class as the label (copied_fields = ['labels']; discard_cases = ['between_thresholds'] only:
// NO visibility discard) and a BoxCoder(10, 10, 5, 5) encode; then a permute + reshape of ten head outputs, a cat, a nonzero, two gathers, the
// focal kernel over every (anchor, class) with its sum, a smooth-L1 over the positives, and autograd's way back through all of it.  Here the
// head output of level l, NHWC [N, nloc_l, ld_l], already IS permute_and_flatten's order inside the level (column a * C + c the logit of
// anchor loc * A + a and class c + 1; columns 4a .. 4a+3 anchor a's deltas), so with n = A * sum nloc_l and off_l = A * sum_{m<l} nloc_m the
// label of (image i, level l, location loc, anchor a) is labels[i * n + off_l + loc * A + a]: the concatenation is addressing.
//
//   abr_retina_targets        2 memsets (the per-ground-truth maxima, n_pos) + 2 launches for the whole batch, as abr_rpn_targets_batched:
//     abr::gt_row_max's pass, then per anchor abr::match_scan_lq<true>, match_index, head_label and box_encode (box_math.h) and the count of
//     labels > 0 (integer atomics, one per workgroup: deterministic).  An image without ground truth: label 0 and zero targets for every
//     anchor, neither of its tables read.
//   abr_retina_loss           1 launch.  A TILE is `rb` consecutive rows (image, location) of one level -- contiguous in the level's cls and
//     reg blocks, about 4096 floats.  A workgroup fetches the tile's rb * A labels into LDS once, then every lane walks the tile 16 bytes at a
//     time: a float4 of logits (anchor and class of its first column by two 32-bit divisions per FOUR logits, stepped from there), then a
//     float4 of deltas = one anchor.  Workgroups stride over the tiles; a workgroup's partial sums are added in a fixed order (its lanes' in
//     tile order, the fixed tree of abr::block_sum), the workgroups' by abr::det_sum_last: no float atomics, the same bits every run.  The
//     last workgroup divides: losses[0] / float(n_pos + N), losses[1] / max(1, n_pos * regress_norm).
//   abr_retina_loss_backward  1 launch over the same tiles: plain 16-byte stores to EVERY element of d_cls and d_reg (one allocation each, the
//     levels back to back; pad columns, ignored anchors and non-positives get 0), so no memset, no scatter, no atomics.  The derivative is
//     recomputed from the logits (abr::focal_deriv, the element of abr_sigmoid_focal_backward) times s = g_cls / float(n_pos + N).
#include <algorithm>

#include "box_math.h"
#include "focal.h"

namespace {

constexpr int MAXL = ABR_MAX_PYRAMID_LEVELS;
constexpr int KT = 256;
constexpr int TILE_FLOATS = 4096;    // a tile's rows hold about this many floats of the wider of the two outputs
constexpr int LAB_CAP = 4096;        // labels of a tile in LDS: rb * A <= max(A, TILE_FLOATS)
constexpr int MAX_GRID = 2048;       // workgroups of the loss kernels (2 partials each: well inside det_ws)

// ------------------------------------------------------------------------------------------------------------------- targets
__global__ __launch_bounds__(KT) void ret_gt_max_kernel(const float* __restrict__ anchors, int n, const float* const* __restrict__ gt_ptrs,
                                                        const int32_t* __restrict__ n_gt, int g_max, unsigned* __restrict__ rowmax) {
    const int i = blockIdx.y;
    abr::gt_row_max(anchors, n, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, gt_ptrs[i], n_gt[i], rowmax + (size_t)i * g_max);
}

__global__ __launch_bounds__(KT) void ret_match_kernel(const float* __restrict__ anchors, int n, const float* const* __restrict__ gt_ptrs,
                                                       const int64_t* const* __restrict__ gt_label_ptrs, const int32_t* __restrict__ n_gt,
                                                       int g_max, float hi, float lo, const unsigned* __restrict__ rowmax, float wx, float wy,
                                                       float ww, float wh, int32_t* __restrict__ labels, float* __restrict__ reg_targets,
                                                       int32_t* __restrict__ n_pos) {
    __shared__ int s_cnt[KT / 64];
    const int i = blockIdx.y, G = n_gt[i];
    const unsigned* rm = rowmax + (size_t)i * g_max;
    int mine = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        int lab = 0;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (G > 0) {     // (head_label reads gt_labels[gi] before it looks at m: an image without ground truth takes no step of this branch)
            const float* gt = gt_ptrs[i];
            const float4 b = reinterpret_cast<const float4*>(anchors)[j];
            const abr::MatchScan s = abr::match_scan_lq<true>(gt, G, b, rm);
            const int m = abr::match_index(s.best, s.bi, s.lq, hi, lo);
            const int gi = m < 0 ? 0 : m;                                               // clamp(min=0)
            lab = (int)abr::head_label(m, gt_label_ptrs[i], gi);
            t = abr::box_encode(reinterpret_cast<const float4*>(gt)[gi], b, wx, wy, ww, wh);
        }
        labels[(size_t)i * n + j] = lab;
        reinterpret_cast<float4*>(reg_targets)[(size_t)i * n + j] = t;
        mine += lab > 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (c) atomicAdd(n_pos, c);
    }
}

// ------------------------------------------------------------------------------------------------------------------- losses
struct RlLevels {                  // by value in the kernel arguments: no device-side table
    const float* cls[MAXL];        // [N, nloc, ldc]
    const float* reg[MAXL];        // [N, nloc, ldr]
    int nloc[MAXL], ldc[MAXL], ldr[MAXL];
    int off[MAXL];                 // first anchor of the level in an image's concatenation
    int rb[MAXL];                  // rows of a tile
    int tile0[MAXL + 1];           // first tile of the level; tile0[L] = all tiles
    long long gc[MAXL], gr[MAXL];  // first float of the level's block in d_cls / d_reg
};

struct RlTile { int l, r0, rows, nloc, off; };

// tile -> its level and rows, its labels into s_lab[rows * A] (row-major); all threads call, a barrier on both sides
__device__ __forceinline__ RlTile rl_tile(const RlLevels& lv, int L, int N, int A, int n, int tile, const int32_t* __restrict__ labels, int* s_lab) {
    RlTile t;
    t.l = 0;
    while (t.l + 1 < L && tile >= lv.tile0[t.l + 1]) t.l++;
    t.nloc = lv.nloc[t.l];
    t.off = lv.off[t.l];
    t.r0 = (tile - lv.tile0[t.l]) * lv.rb[t.l];
    t.rows = min(lv.rb[t.l], N * t.nloc - t.r0);
    __syncthreads();               // the previous tile's readers are done with s_lab
    for (int idx = threadIdx.x; idx < t.rows * A; idx += KT) {
        const int rr = idx / A, a = idx - rr * A, r = t.r0 + rr;
        const int i = r / t.nloc, loc = r - i * t.nloc;
        s_lab[idx] = labels[(size_t)i * n + t.off + loc * A + a];
    }
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(KT) void ret_loss_kernel(RlLevels lv, int L, int N, int A, int C, int n, const int32_t* __restrict__ labels,
                                                      const float* __restrict__ reg_targets, const int32_t* __restrict__ n_pos, float gamma,
                                                      float alpha, float beta, float regress_norm, float* __restrict__ losses, const abr::DetWs ws) {
    __shared__ int s_lab[LAB_CAP];
    __shared__ float sm[KT / 64];
    const int AC = A * C, tiles = lv.tile0[L];
    float acc_c = 0.f, acc_r = 0.f;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const RlTile t = rl_tile(lv, L, N, A, n, tile, labels, s_lab);
        {
            const int ldc = lv.ldc[t.l], qpr = ldc >> 2, nq = t.rows * qpr;
            const float4* x4 = reinterpret_cast<const float4*>(lv.cls[t.l] + (size_t)t.r0 * ldc);
            for (int q = threadIdx.x; q < nq; q += KT) {
                const int rr = q / qpr, col = (q - rr * qpr) << 2;
                if (col >= AC) continue;                       // pad columns are never read
                const float4 v = x4[q];
                const float xs[4] = {v.x, v.y, v.z, v.w};
                const int* lab = s_lab + rr * A;
                int a = col / C, c = col - a * C;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (col + k < AC) {
                        const int tl = lab[a];
                        if (tl >= 0) acc_c += abr::focal_value<float>(xs[k], tl, c, gamma, alpha);
                        if (++c == C) { c = 0; a++; }
                    }
                }
            }
        }
        {
            const int ldr = lv.ldr[t.l], qpr = ldr >> 2, nq = t.rows * qpr;
            const float4* r4 = reinterpret_cast<const float4*>(lv.reg[t.l] + (size_t)t.r0 * ldr);
            for (int q = threadIdx.x; q < nq; q += KT) {
                const int rr = q / qpr, a = q - rr * qpr;
                if (a >= A || s_lab[rr * A + a] <= 0) continue;
                const int r = t.r0 + rr, i = r / t.nloc, loc = r - i * t.nloc;
                const float4 v = r4[q], tg = reinterpret_cast<const float4*>(reg_targets)[(size_t)i * n + t.off + loc * A + a];
                float g;
                acc_r += abr::sl1(v.x - tg.x, beta, &g);
                acc_r += abr::sl1(v.y - tg.y, beta, &g);
                acc_r += abr::sl1(v.z - tg.z, beta, &g);
                acc_r += abr::sl1(v.w - tg.w, beta, &g);
            }
        }
    }
    const float in[2] = {abr::block_sum<KT / 64>(acc_c, sm), abr::block_sum<KT / 64>(acc_r, sm)};
    float tot[2];
    if (abr::det_sum_last<2>(in, ws, tot) && threadIdx.x == 0) {
        const int np = *n_pos;
        losses[0] = tot[0] / (float)(np + N);
        losses[1] = tot[1] / fmaxf(1.f, (float)np * regress_norm);
    }
}

__global__ __launch_bounds__(KT) void ret_loss_bwd_kernel(RlLevels lv, int L, int N, int A, int C, int n, const int32_t* __restrict__ labels,
                                                          const float* __restrict__ reg_targets, const int32_t* __restrict__ n_pos, float gamma,
                                                          float alpha, float beta, float regress_norm, const float* __restrict__ g_cls,
                                                          const float* __restrict__ g_reg, float* __restrict__ d_cls, float* __restrict__ d_reg) {
    __shared__ int s_lab[LAB_CAP];
    const int AC = A * C, tiles = lv.tile0[L];
    const int np = *n_pos;
    const float s = *g_cls / (float)(np + N);
    const float sr = *g_reg / fmaxf(1.f, (float)np * regress_norm);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const RlTile t = rl_tile(lv, L, N, A, n, tile, labels, s_lab);
        {
            const int ldc = lv.ldc[t.l], qpr = ldc >> 2, nq = t.rows * qpr;
            const float4* x4 = reinterpret_cast<const float4*>(lv.cls[t.l] + (size_t)t.r0 * ldc);
            float4* d4 = reinterpret_cast<float4*>(d_cls + lv.gc[t.l] + (size_t)t.r0 * ldc);
            for (int q = threadIdx.x; q < nq; q += KT) {
                const int rr = q / qpr, col = (q - rr * qpr) << 2;
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (col < AC) {
                    const float4 v = x4[q];
                    const float xs[4] = {v.x, v.y, v.z, v.w};
                    const int* lab = s_lab + rr * A;
                    int a = col / C, c = col - a * C;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (col + k < AC) {
                            const int tl = lab[a];
                            if (tl >= 0) o[k] = abr::focal_deriv<float>(xs[k], tl, c, gamma, alpha) * s;
                            if (++c == C) { c = 0; a++; }
                        }
                    }
                }
                d4[q] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        {
            const int ldr = lv.ldr[t.l], qpr = ldr >> 2, nq = t.rows * qpr;
            const float4* r4 = reinterpret_cast<const float4*>(lv.reg[t.l] + (size_t)t.r0 * ldr);
            float4* d4 = reinterpret_cast<float4*>(d_reg + lv.gr[t.l] + (size_t)t.r0 * ldr);
            for (int q = threadIdx.x; q < nq; q += KT) {
                const int rr = q / qpr, a = q - rr * qpr;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a < A && s_lab[rr * A + a] > 0) {
                    const int r = t.r0 + rr, i = r / t.nloc, loc = r - i * t.nloc;
                    const float4 v = r4[q], tg = reinterpret_cast<const float4*>(reg_targets)[(size_t)i * n + t.off + loc * A + a];
                    (void)abr::sl1(v.x - tg.x, beta, &o.x);
                    (void)abr::sl1(v.y - tg.y, beta, &o.y);
                    (void)abr::sl1(v.z - tg.z, beta, &o.z);
                    (void)abr::sl1(v.w - tg.w, beta, &o.w);
                    o.x *= sr; o.y *= sr; o.z *= sr; o.w *= sr;
                }
                d4[q] = o;
            }
        }
    }
}

// the host tables -> the kernels' by-value argument; checks what both entries check.  *n_out = anchors per image
int fill_levels(const char* name, RlLevels& lv, const float* const* cls, const int* ldc, const float* const* reg, const int* ldr, const int* nloc,
                int L, int N, int A, int C, int* n_out, long long* cls_floats, long long* reg_floats) {
    ABR_REQUIRE(L >= 1 && L <= MAXL, "%s: L = %d levels, need 1 .. %d", name, L, MAXL);
    ABR_REQUIRE(N >= 0 && A >= 1 && C >= 1, "%s: bad N, A or C", name);
    ABR_REQUIRE(A <= LAB_CAP && (long long)A * C <= 0x7FFFFFFF, "%s: A = %d anchors per location, at most %d", name, A, LAB_CAP);
    ABR_REQUIRE(cls && ldc && reg && ldr && nloc, "%s: null level table", name);
    long long off = 0, gc = 0, gr = 0, tiles = 0;
    for (int l = 0; l < MAXL; l++) {
        const int s = l < L ? l : 0;     // unused entries repeat level 0
        ABR_REQUIRE(nloc[s] >= 1, "%s: level %d: nloc = %d", name, s, nloc[s]);
        ABR_REQUIRE(ldc[s] >= (long long)A * C && ldc[s] % 4 == 0, "%s: level %d: ldc = %d, need a multiple of 4 that holds A * C = %lld logits", name, s,
                    ldc[s], (long long)A * C);
        ABR_REQUIRE(ldr[s] >= 4LL * A && ldr[s] % 4 == 0, "%s: level %d: ldr = %d, need a multiple of 4 that holds 4A = %lld deltas", name, s, ldr[s],
                    4LL * A);
        ABR_REQUIRE(N == 0 || (cls[s] && reg[s]), "%s: level %d: null pointer", name, s);
        ABR_REQUIRE(((reinterpret_cast<uintptr_t>(cls[s]) | reinterpret_cast<uintptr_t>(reg[s])) & 15) == 0,
                    "%s: level %d: the head outputs must be 16-byte aligned", name, s);
        ABR_REQUIRE((long long)std::max(N, 1) * nloc[s] * std::max(ldc[s], ldr[s]) <= 0x7FFFFFFF, "%s: level %d does not fit int32", name, s);
        lv.cls[l] = cls[s];
        lv.reg[l] = reg[s];
        lv.nloc[l] = nloc[s];
        lv.ldc[l] = ldc[s];
        lv.ldr[l] = ldr[s];
        lv.off[l] = (int)off;
        lv.gc[l] = gc;
        lv.gr[l] = gr;
        lv.rb[l] = std::max(1, TILE_FLOATS / std::max(ldc[s], ldr[s]));
        lv.tile0[l] = (int)tiles;
        if (l < L) {
            off += (long long)nloc[l] * A;
            gc += (long long)N * nloc[l] * ldc[l];
            gr += (long long)N * nloc[l] * ldr[l];
            tiles += ((long long)N * nloc[l] + lv.rb[l] - 1) / lv.rb[l];
            ABR_REQUIRE((long long)std::max(N, 1) * off <= 0x7FFFFFFF, "%s: the batch's N * n anchors do not fit int32", name);
        }
    }
    lv.tile0[MAXL] = (int)tiles;     // (entries L .. MAXL all hold the total)
    *n_out = (int)off;
    *cls_floats = gc;
    *reg_floats = gr;
    return ABR_OK;
}

}  // namespace

extern "C" int abr_retina_targets(const float* anchors, int n, int N, const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs,
                                  const int32_t* n_gt, int g_max, float hi, float lo, float wx, float wy, float ww, float wh, int32_t* labels,
                                  float* reg_targets, int32_t* n_pos, void* stream) {
    ABR_REQUIRE(n >= 0 && N >= 0 && g_max >= 0, "retina_targets: bad sizes");
    ABR_REQUIRE((long long)std::max(N, 1) * n <= 0x7FFFFFFF, "retina_targets: N * n = %lld anchors do not fit int32", (long long)N * n);
    ABR_REQUIRE(N <= 65535, "retina_targets: N = %d images, at most 65535", N);
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(n_pos, "retina_targets: null pointer");
    hipStream_t st = abr::as_stream(stream);
    ABR_REQUIRE(n == 0 || (anchors && gt_ptrs && gt_label_ptrs && n_gt && labels && reg_targets), "retina_targets: null pointer");
    ABR_REQUIRE(((reinterpret_cast<uintptr_t>(anchors) | reinterpret_cast<uintptr_t>(reg_targets)) & 15) == 0,
                "retina_targets: anchors and reg_targets must be 16-byte aligned");
    unsigned* rowmax = nullptr;
    if (n > 0) {
        rowmax = static_cast<unsigned*>(abr::scratch(abr::SCRATCH_RETINA_TARGETS, st, 4 * (size_t)N * std::max(g_max, 1)));
        ABR_REQUIRE(rowmax, "retina_targets: scratch allocation failed");
    }
    if (hipMemsetAsync(n_pos, 0, sizeof(int32_t), st) != hipSuccess) return ABR_E_LAUNCH;
    if (n == 0) return ABR_OK;
    if (hipMemsetAsync(rowmax, 0, 4 * (size_t)N * std::max(g_max, 1), st) != hipSuccess) return ABR_E_LAUNCH;
    ret_gt_max_kernel<<<dim3(std::min(abr::cdiv(n, 1024), 64u), N), KT, 0, st>>>(anchors, n, gt_ptrs, n_gt, g_max, rowmax);
    ret_match_kernel<<<dim3(std::min(abr::cdiv(n, KT), 1024u), N), KT, 0, st>>>(anchors, n, gt_ptrs, gt_label_ptrs, n_gt, g_max, hi, lo, rowmax, wx, wy,
                                                                               ww, wh, labels, reg_targets, n_pos);
    ABR_CHECK_LAUNCH("retina_targets");
    return ABR_OK;
}

extern "C" int abr_retina_loss(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host,
                               const int* nloc_host, int L, int N, int A, int C, const int32_t* labels, const float* reg_targets,
                               const int32_t* n_pos, float gamma, float alpha, float beta, float regress_norm, float* losses, void* stream) {
    RlLevels lv;
    int n;
    long long cf, rf;
    const int rc = fill_levels("retina_loss", lv, cls_host, ldc_host, reg_host, ldr_host, nloc_host, L, N, A, C, &n, &cf, &rf);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(beta > 0.f, "retina_loss: beta = %g, need > 0", (double)beta);
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(labels && reg_targets && n_pos && losses, "retina_loss: null pointer");
    ABR_REQUIRE((reinterpret_cast<uintptr_t>(reg_targets) & 15) == 0, "retina_loss: reg_targets must be 16-byte aligned");
    hipStream_t st = abr::as_stream(stream);
    const unsigned grid = (unsigned)std::min(lv.tile0[L], MAX_GRID);
    const abr::DetWs ws = abr::det_ws(st, 2 * (size_t)grid);
    ABR_REQUIRE(ws.part, "retina_loss: scratch allocation failed");
    ret_loss_kernel<<<grid, KT, 0, st>>>(lv, L, N, A, C, n, labels, reg_targets, n_pos, gamma, alpha, beta, regress_norm, losses, ws);
    ABR_CHECK_LAUNCH("retina_loss");
    return ABR_OK;
}

extern "C" int abr_retina_loss_backward(const float* const* cls_host, const int* ldc_host, const float* const* reg_host, const int* ldr_host,
                                        const int* nloc_host, int L, int N, int A, int C, const int32_t* labels, const float* reg_targets,
                                        const int32_t* n_pos, float gamma, float alpha, float beta, float regress_norm, const float* g_cls,
                                        const float* g_reg, float* d_cls, float* d_reg, void* stream) {
    RlLevels lv;
    int n;
    long long cf, rf;
    const int rc = fill_levels("retina_loss_backward", lv, cls_host, ldc_host, reg_host, ldr_host, nloc_host, L, N, A, C, &n, &cf, &rf);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(beta > 0.f, "retina_loss_backward: beta = %g, need > 0", (double)beta);
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(labels && reg_targets && n_pos && g_cls && g_reg && d_cls && d_reg, "retina_loss_backward: null pointer");
    ABR_REQUIRE(((reinterpret_cast<uintptr_t>(reg_targets) | reinterpret_cast<uintptr_t>(d_cls) | reinterpret_cast<uintptr_t>(d_reg)) & 15) == 0,
                "retina_loss_backward: reg_targets, d_cls and d_reg must be 16-byte aligned");
    hipStream_t st = abr::as_stream(stream);
    const unsigned grid = (unsigned)std::min(lv.tile0[L], MAX_GRID);
    ret_loss_bwd_kernel<<<grid, KT, 0, st>>>(lv, L, N, A, C, n, labels, reg_targets, n_pos, gamma, alpha, beta, regress_norm, g_cls, g_reg, d_cls,
                                             d_reg);
    ABR_CHECK_LAUNCH("retina_loss_backward");
    return ABR_OK;
}
