// Mask head (MODEL.MASK_ON, MaskRCNNC4Predictor) -- the memory-bound kernels around its two contractions, which run on the conv planner:
//   positive-RoI compaction, row gather and its backward      modeling/roi_heads/mask_head/mask_head.py:13-33, 62-79
//   mask targets (crop + bilinear resize of the matched mask)  mask_head/loss.py:11-100, structures/segmentation_mask.py:92-135
//   depth-to-space + bias + ReLU of the 2x2 stride-2 deconv    mask_head/roi_mask_predictors.py:10-32
//   mask loss (BCE with logits on channel labels[p]) + grad    mask_head/loss.py:102-128
//   eval: sigmoid of channel labels[i], paste into the image   mask_head/inference.py:27-61, 91-159
// Activations are NHWC; every access along C is 16 bytes wide.
#include <algorithm>

#include "common.h"
#include "mask_bilinear.h"
#include "mask_match.h"

namespace {

// ------------------------------------------------------------------------------------------------
// positives of the sampled set, compacted in ascending row order (one workgroup: K is a few thousand rows)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void mask_compact_kernel(const int64_t* __restrict__ labels, int K, int P_max, int64_t* __restrict__ pos_rows,
                                                            int64_t* __restrict__ pos_labels, int64_t* __restrict__ inv, int* __restrict__ n_pos) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int start = 0; start < K; start += 1024) {
        const int i = start + tid;
        const int64_t l = i < K ? labels[i] : 0;
        const bool flag = l > 0;
        const unsigned long long b = __ballot(flag);
        const int prefix = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) s_wave[wv] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int c = s_wave[w];
            off += w < wv ? c : 0;
            tot += c;
        }
        if (i < K) {
            const int p = base + off + prefix;
            const bool take = flag && p < P_max;
            if (take) {
                pos_rows[p] = i;
                pos_labels[p] = l;
            }
            inv[i] = take ? p : -1;
        }
        base += tot;
    }
    const int n = min(base, P_max);
    for (int p = n + tid; p < P_max; p += 1024) {
        pos_rows[p] = -1;
        pos_labels[p] = -1;
    }
    if (tid == 0) *n_pos = n;
}

// out[p] = x[rows[p]] (rows[p] < 0: zeros).  The backward is the same kernel over the inverse map: every row of the gradient is written once.
__global__ __launch_bounds__(256) void mask_rows_kernel(const float4* __restrict__ x, const int64_t* __restrict__ rows, int n_src, int64_t row4,
                                                        float4* __restrict__ out) {
    const int p = blockIdx.y;
    const int64_t r = rows[p];
    const bool ok = r >= 0 && r < n_src;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < row4; i += (int64_t)gridDim.x * 256)
        out[(int64_t)p * row4 + i] = ok ? x[r * row4 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------
// mask targets
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ int round_to_int(const float v) {   // Python round() of a float: half to even
    return (int)fminf(fmaxf(rintf(v), -1.0e9f), 1.0e9f);
}

template <typename T>
__global__ __launch_bounds__(256) void mask_targets_kernel(const T* const* __restrict__ mask_ptrs, const int32_t* __restrict__ dims,
                                                           const float* const* __restrict__ gt_ptrs, const float* __restrict__ rois,
                                                           const int64_t* __restrict__ pos_rows, int K, int N, int M, float* __restrict__ out) {
    __shared__ int s[8];
    const int p = blockIdx.x;
    const int64_t row = pos_rows[p];
    float* o = out + (int64_t)p * M * M;
    int img = -1;
    if (row >= 0 && row < K) img = (int)rois[row * 5];
    if (img < 0 || img >= N || dims[img * 3] <= 0) {   // padding row
        for (int i = threadIdx.x; i < M * M; i += 256) o[i] = 0.f;
        return;
    }
    const int G = dims[img * 3], H = dims[img * 3 + 1], W = dims[img * 3 + 2];
    if (threadIdx.x == 0) {
        const float4 b = make_float4(rois[row * 5 + 1], rois[row * 5 + 2], rois[row * 5 + 3], rois[row * 5 + 4]);
        const float4* gt = reinterpret_cast<const float4*>(gt_ptrs[img]);
        const int bi = abr::mask_match_gt(gt, G, b);      // first maximum IoU (mask_match.h)
        // BinaryMaskList.crop (segmentation_mask.py:92-111)
        int xmin = round_to_int(b.x), ymin = round_to_int(b.y), xmax = round_to_int(b.z), ymax = round_to_int(b.w);
        xmin = min(max(xmin, 0), W - 1);
        ymin = min(max(ymin, 0), H - 1);
        xmax = min(max(xmax, 0), W);
        ymax = min(max(ymax, 0), H);
        xmax = max(xmax, xmin + 1);
        ymax = max(ymax, ymin + 1);
        s[0] = bi; s[1] = xmin; s[2] = ymin; s[3] = xmax - xmin; s[4] = ymax - ymin;
    }
    __syncthreads();
    const int xmin = s[1], ymin = s[2], cw = s[3], ch = s[4];
    const T* m = mask_ptrs[img] + (int64_t)s[0] * H * W;
    const float sh = (float)ch / (float)M, sw = (float)cw / (float)M;
    const bool four_weight = bilinear_four_weight_path(M, M);   // torch's resize changes its operation order beyond M = 64 (mask_bilinear.h)
    for (int i = threadIdx.x; i < M * M; i += 256) {
        const int oy = i / M, ox = i - oy * M;
        int y0, y1, x0, x1;
        float ly, lx;
        bilinear_tap(sh, oy, ch, y0, y1, ly);
        bilinear_tap(sw, ox, cw, x0, x1, lx);
        const T* r0 = m + (int64_t)(ymin + y0) * W + xmin;
        const T* r1 = m + (int64_t)(ymin + y1) * W + xmin;
        const float v00 = (float)r0[x0], v01 = (float)r0[x1], v10 = (float)r1[x0], v11 = (float)r1[x1];
        float v = four_weight ? bilinear_mix(v00, v01, v10, v11, lx, ly) : bilinear_mix_separable(v00, v01, v10, v11, lx, ly);
        if (sizeof(T) == 1) v = (float)(unsigned char)(int)v;    // .type_as(uint8 masks): truncation
        o[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// ConvTranspose2d(k=2, s=2, p=0) as GEMM + depth-to-space: y [P,h,w,(dy,dx,co)] -> out [P,2h,2w,co] = relu(y + bias[co])
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void d2s_bias_relu_kernel(const float4* __restrict__ y, const float4* __restrict__ bias, int64_t total4, int h,
                                                            int w, int c4, float4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % c4);
        int64_t t = i / c4;
        const int X = (int)(t % (2 * w));
        t /= 2 * w;
        const int Y = (int)(t % (2 * h));
        const int64_t n = t / (2 * h);
        const int q = (Y & 1) * 2 + (X & 1);
        const float4 v = y[(((n * h + (Y >> 1)) * w + (X >> 1)) * 4 + q) * c4 + c];
        const float4 b = bias[c];
        out[i] = make_float4(abr::relu_f(v.x + b.x), abr::relu_f(v.y + b.y), abr::relu_f(v.z + b.z), abr::relu_f(v.w + b.w));
    }
}

// gy [P,h,w,(dy,dx,co)] = out > 0 ? g : 0 (ReLU mask + space-to-depth); the bias gradient is the column sum of gy seen as [P h w 4, co]
__global__ __launch_bounds__(256) void d2s_bias_relu_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ out, int64_t total4, int h,
                                                                int w, int c4, float4* __restrict__ gy) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % c4);
        int64_t t = i / c4;
        const int q = (int)(t & 3);
        t >>= 2;
        const int x = (int)(t % w);
        t /= w;
        const int yy = (int)(t % h);
        const int64_t n = t / h;
        const int64_t src = ((n * 2 * h + 2 * yy + (q >> 1)) * 2 * w + 2 * x + (q & 1)) * c4 + c;
        const float4 gv = g[src], ov = out[src];
        gy[i] = make_float4(ov.x > 0.f ? gv.x : 0.f, ov.y > 0.f ? gv.y : 0.f, ov.z > 0.f ? gv.z : 0.f, ov.w > 0.f ? gv.w : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// mask loss: mean over (positive rows) x M x M of BCE-with-logits on channel labels[p], and its gradient
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_loss_kernel(const float4* __restrict__ logits, int ld4, int Kc, const int64_t* __restrict__ labels,
                                                        const float* __restrict__ targets, int64_t total4, int MM, const int* __restrict__ n_pos,
                                                        int P, float* __restrict__ loss_out, float gscale, float4* __restrict__ grad,
                                                        const abr::DetWs ws) {
    __shared__ float sm[4];
    const int np = n_pos ? *n_pos : P;
    const float inv = np > 0 ? 1.f / ((float)np * (float)MM) : 0.f;
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % ld4);
        const int64_t e = i / ld4;          // (row, pixel)
        const int64_t l = labels[e / MM];
        float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l > 0 && l < Kc && (int)(l >> 2) == c) {
            const float4 xv4 = logits[i];
            const int k = (int)(l & 3);
            const float xv = k == 0 ? xv4.x : (k == 1 ? xv4.y : (k == 2 ? xv4.z : xv4.w));
            const float tv = targets[e];
            acc += fmaxf(xv, 0.f) - xv * tv + log1pf(expf(-fabsf(xv)));
            const float gk = (1.f / (1.f + expf(-xv)) - tv) * inv * gscale;
            if (k == 0) gv.x = gk; else if (k == 1) gv.y = gk; else if (k == 2) gv.z = gk; else gv.w = gk;
        }
        if (grad) grad[i] = gv;
    }
    acc = abr::block_sum<4>(acc, sm);
    if (ws.part) {
        const float in[1] = {acc};
        float tot[1];
        if (abr::det_sum_last<1>(in, ws, tot) && threadIdx.x == 0) *loss_out = tot[0] * inv;
    } else if (threadIdx.x == 0) {
        atomicAdd(loss_out, acc * inv);
    }
}

// ------------------------------------------------------------------------------------------------
// eval
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_select_sigmoid_kernel(const float* __restrict__ logits, int ldk, int Kc, const int64_t* __restrict__ labels,
                                                                  int64_t total, int MM, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t l = labels[i / MM];
        out[i] = (l >= 0 && l < Kc) ? 1.f / (1.f + expf(-logits[i * ldk + l])) : 0.f;
    }
}

// paste_mask_in_image (inference.py:119-159) for one canvas pixel of detection d: pad the M x M probabilities by 1, expand the box by
// (M + 2) / M, truncate it to int32, resize the padded mask to the box (bilinear, align_corners=False), threshold, clip to the canvas
#pragma clang fp contract(off)
__device__ __forceinline__ unsigned paste_pixel(const float* __restrict__ prob, const float4 b, const int M, const float scale, const int im_h,
                                                const int im_w, const float thresh, const int y, const int x) {
    float w_half = (b.z - b.x) * 0.5f, h_half = (b.w - b.y) * 0.5f;
    const float x_c = (b.z + b.x) * 0.5f, y_c = (b.w + b.y) * 0.5f;
    w_half *= scale;
    h_half *= scale;
    const int bx0 = (int)(x_c - w_half), bx2 = (int)(x_c + w_half), by1 = (int)(y_c - h_half), by3 = (int)(y_c + h_half);
    const int w = max(bx2 - bx0 + 1, 1), h = max(by3 - by1 + 1, 1);
    const int x_0 = max(bx0, 0), x_1 = min(bx2 + 1, im_w), y_0 = max(by1, 0), y_1 = min(by3 + 1, im_h);
    if (x < x_0 || x >= x_1 || y < y_0 || y >= y_1) return 0u;
    const int Mp = M + 2;
    int i0, i1, j0, j1;
    float ly, lx;
    bilinear_tap((float)Mp / (float)h, y - by1, Mp, i0, i1, ly);
    bilinear_tap((float)Mp / (float)w, x - bx0, Mp, j0, j1, lx);
    auto at = [&](const int i, const int j) { return (i >= 1 && i <= M && j >= 1 && j <= M) ? prob[(i - 1) * M + (j - 1)] : 0.f; };
    const float v = bilinear_mix(at(i0, j0), at(i0, j1), at(i1, j0), at(i1, j1), lx, ly);
    return v > thresh ? 1u : 0u;
}

__global__ __launch_bounds__(256) void mask_paste_kernel(const float* __restrict__ prob, const float* __restrict__ boxes, int64_t total, int M,
                                                         float scale, int im_h, int im_w, float thresh, uint8_t* __restrict__ out) {
    const int64_t hw = (int64_t)im_h * im_w;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c * 4 < total; c += (int64_t)gridDim.x * 256) {
        unsigned pk = 0u;
        const int n = (int)min((int64_t)4, total - c * 4);
        for (int j = 0; j < n; j++) {
            const int64_t i = c * 4 + j;
            const int64_t d = i / hw;
            const int64_t r = i - d * hw;
            const int y = (int)(r / im_w), x = (int)(r - (int64_t)y * im_w);
            const float4 b = reinterpret_cast<const float4*>(boxes)[d];
            pk |= paste_pixel(prob + d * M * M, b, M, scale, im_h, im_w, thresh, y, x) << (8 * j);
        }
        if (n == 4) reinterpret_cast<unsigned*>(out)[c] = pk;
        else for (int j = 0; j < n; j++) out[c * 4 + j] = (uint8_t)((pk >> (8 * j)) & 0xFFu);
    }
}

unsigned grid_for(int64_t work, unsigned cap = 4096u) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, cap)); }

}  // namespace

extern "C" int abr_mask_compact_pos(const int64_t* labels, int K, int P_max, int64_t* pos_rows, int64_t* pos_labels, int64_t* inv, int32_t* n_pos,
                                    void* stream) {
    ABR_REQUIRE(K >= 0 && P_max >= 0 && n_pos, "mask_compact_pos: bad args");
    ABR_REQUIRE((K == 0 || (labels && inv)) && (P_max == 0 || (pos_rows && pos_labels)), "mask_compact_pos: null pointer");
    mask_compact_kernel<<<1, 1024, 0, abr::as_stream(stream)>>>(labels, K, P_max, pos_rows, pos_labels, inv, n_pos);
    ABR_CHECK_LAUNCH("mask_compact_pos");
    return ABR_OK;
}

extern "C" int abr_mask_gather_rows(const float* x, const int64_t* rows, int n_src, int n_out, int64_t row_floats, float* out, void* stream) {
    ABR_REQUIRE(n_src >= 0 && n_out >= 0 && row_floats > 0 && row_floats % 4 == 0, "mask_gather_rows: bad args (row length must be a multiple of 4)");
    if (n_out == 0) return ABR_OK;
    ABR_REQUIRE(rows && out && (x || n_src == 0), "mask_gather_rows: null pointer");
    ABR_REQUIRE(n_out <= 65535, "mask_gather_rows: more than 65535 output rows");
    const int64_t row4 = row_floats / 4;
    mask_rows_kernel<<<dim3(grid_for(row4, 64u), n_out), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(x), rows, n_src, row4,
                                                                                         reinterpret_cast<float4*>(out));
    ABR_CHECK_LAUNCH("mask_gather_rows");
    return ABR_OK;
}

extern "C" int abr_mask_targets(const void* const* mask_ptrs, const int32_t* mask_dims, int is_u8, const float* const* gt_ptrs, const float* rois,
                                const int64_t* pos_rows, int P_max, int K, int N, int M, float* out, void* stream) {
    ABR_REQUIRE(P_max >= 0 && K >= 0 && N > 0 && M > 0 && M <= 256, "mask_targets: bad args");
    if (P_max == 0) return ABR_OK;
    ABR_REQUIRE(mask_ptrs && mask_dims && gt_ptrs && rois && pos_rows && out, "mask_targets: null pointer");
    hipStream_t st = abr::as_stream(stream);
    if (is_u8)
        mask_targets_kernel<uint8_t><<<P_max, 256, 0, st>>>(reinterpret_cast<const uint8_t* const*>(mask_ptrs), mask_dims, gt_ptrs, rois, pos_rows, K, N, M, out);
    else
        mask_targets_kernel<float><<<P_max, 256, 0, st>>>(reinterpret_cast<const float* const*>(mask_ptrs), mask_dims, gt_ptrs, rois, pos_rows, K, N, M, out);
    ABR_CHECK_LAUNCH("mask_targets");
    return ABR_OK;
}

extern "C" int abr_mask_d2s_bias_relu(const float* y, const float* bias, int P, int h, int w, int Cm, float* out, void* stream) {
    ABR_REQUIRE(P >= 0 && h > 0 && w > 0 && Cm > 0 && Cm % 4 == 0, "mask_d2s_bias_relu: bad args (channels must be a multiple of 4)");
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(y && bias && out, "mask_d2s_bias_relu: null pointer");
    const int64_t total4 = (int64_t)P * h * w * Cm;    // = P * 2h * 2w * Cm / 4
    d2s_bias_relu_kernel<<<grid_for(total4), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(y), reinterpret_cast<const float4*>(bias),
                                                                              total4, h, w, Cm / 4, reinterpret_cast<float4*>(out));
    ABR_CHECK_LAUNCH("mask_d2s_bias_relu");
    return ABR_OK;
}

extern "C" int abr_mask_d2s_bias_relu_backward(const float* g, const float* out, int P, int h, int w, int Cm, float* gy, void* stream) {
    ABR_REQUIRE(P >= 0 && h > 0 && w > 0 && Cm > 0 && Cm % 4 == 0, "mask_d2s_bias_relu_backward: bad args (channels must be a multiple of 4)");
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(g && out && gy, "mask_d2s_bias_relu_backward: null pointer");
    const int64_t total4 = (int64_t)P * h * w * Cm;
    d2s_bias_relu_bwd_kernel<<<grid_for(total4), 256, 0, abr::as_stream(stream)>>>(reinterpret_cast<const float4*>(g), reinterpret_cast<const float4*>(out),
                                                                                  total4, h, w, Cm / 4, reinterpret_cast<float4*>(gy));
    ABR_CHECK_LAUNCH("mask_d2s_bias_relu_backward");
    return ABR_OK;
}

extern "C" int abr_mask_loss(const float* logits, int ldk, int Kc, const int64_t* labels, const float* targets, int P, int MM, const int32_t* n_pos,
                             float* loss_out, float gscale, float* grad, void* stream) {
    ABR_REQUIRE(P >= 0 && MM > 0 && ldk > 0 && ldk % 4 == 0 && Kc > 0 && Kc <= ldk && loss_out, "mask_loss: bad args (row stride must be a multiple of 4)");
    hipStream_t st = abr::as_stream(stream);
    if (hipMemsetAsync(loss_out, 0, sizeof(float), st) != hipSuccess) {
        abr::set_error("mask_loss: hipMemsetAsync failed");
        return ABR_E_LAUNCH;
    }
    if (P == 0) return ABR_OK;
    ABR_REQUIRE(logits && labels && targets, "mask_loss: null pointer");
    const int64_t total4 = (int64_t)P * MM * (ldk / 4);
    const unsigned grid = grid_for(total4, 1024u);
    mask_loss_kernel<<<grid, 256, 0, st>>>(reinterpret_cast<const float4*>(logits), ldk / 4, Kc, labels, targets, total4, MM, n_pos, P, loss_out, gscale,
                                           reinterpret_cast<float4*>(grad), abr::det_ws(st, grid));
    ABR_CHECK_LAUNCH("mask_loss");
    return ABR_OK;
}

extern "C" int abr_mask_select_sigmoid(const float* logits, int ldk, int Kc, const int64_t* labels, int D, int MM, float* out, void* stream) {
    ABR_REQUIRE(D >= 0 && MM > 0 && ldk > 0 && Kc > 0 && Kc <= ldk, "mask_select_sigmoid: bad args");
    if (D == 0) return ABR_OK;
    ABR_REQUIRE(logits && labels && out, "mask_select_sigmoid: null pointer");
    const int64_t total = (int64_t)D * MM;
    mask_select_sigmoid_kernel<<<grid_for(total), 256, 0, abr::as_stream(stream)>>>(logits, ldk, Kc, labels, total, MM, out);
    ABR_CHECK_LAUNCH("mask_select_sigmoid");
    return ABR_OK;
}

extern "C" int abr_mask_paste(const float* prob, const float* boxes, int D, int M, int im_h, int im_w, float thresh, uint8_t* out, void* stream) {
    ABR_REQUIRE(D >= 0 && M > 0 && im_h > 0 && im_w > 0, "mask_paste: bad args");
    ABR_REQUIRE(thresh >= 0.f, "mask_paste: a negative threshold (the reference's unthresholded debug output) is not supported");
    if (D == 0) return ABR_OK;
    ABR_REQUIRE(prob && boxes && out, "mask_paste: null pointer");
    const int64_t total = (int64_t)D * im_h * im_w;
    const float scale = (float)((double)(M + 2) / (double)M);    // expand_masks: float(M + 2 * padding) / M, then a float32 multiply
    mask_paste_kernel<<<grid_for((total + 3) / 4, 16384u), 256, 0, abr::as_stream(stream)>>>(prob, boxes, total, M, scale, im_h, im_w, thresh, out);
    ABR_CHECK_LAUNCH("mask_paste");
    return ABR_OK;
}
