// ROIPool and deformable PS-RoI pooling for gfx950: the two RoI poolers of the reference that have CUDA kernels only.
//
// Reference semantics: maskrcnn_benchmark/csrc/cuda/ROIPool_cuda.cu:16-108 and csrc/cuda/deform_pool_kernel_cuda.cu:31-264.
//
// Design, as csrc/roi_align.hip:
//   * the native layout is NHWC: a bin's pixels (ROIPool) and a sample's four taps (PS-RoI, group_size 1) are contiguous channel vectors,
//     read as 16 B per lane with the lanes of a wave along the channels of ONE bin -- the bin's geometry is wave-uniform;
//   * the geometry is compiled with FP contraction off, one rounding per operation in the reference's order: ROIPool's bin borders are
//     floor / ceil of fp32 products (length 57 over 7 bins ends the last bin at 58) and stay that way;
//   * the NCHW kernels are the `_C` parity route, one thread per output with pw fastest, like roi_align_fwd_nchw;
//   * gradients of the map go through fp32 atomics shaped as contiguous channel runs of one bin (NHWC).  The offset and mask-logit gradients of
//     PS-RoI pooling have one owner each: the workgroup of a (RoI, part cell) walks the cell's bins, classes, channels and samples in a fixed
//     order and sums across its threads with a fixed tree -- no atomics, bit-reproducible.
// Bound: HBM / L2 on the forward kernels, the chip-wide float-atomic rate on the backward kernels; figures in DESIGN.md section 4.
#include <float.h>
#include <limits.h>

#include "common.h"

namespace {

template <int VEC>
struct VecT;
template <>
struct VecT<4> { using type = float4; using itype = int4; };
template <>
struct VecT<1> { using type = float; using itype = int; };

// =====================================================================================================================================
// ROIPool
// =====================================================================================================================================
struct PoolBin { int b, hs, he, ws, we; };

// ROIPool_cuda.cu:28-56 for T = float and T = double: round half away from zero, +1 lengths, bin = len / P in T, floor / ceil of ONE rounded
// product each, the RoI start added afterwards, clipped to the map
#pragma clang fp contract(off)
template <typename T>
__device__ __forceinline__ PoolBin pool_bin(const T* __restrict__ r, T scale, int H, int W, int PH, int PW, int ph, int pw) {
    PoolBin q;
    q.b = (int)r[0];
    const int sw = (int)round(r[1] * scale), sh = (int)round(r[2] * scale), ew = (int)round(r[3] * scale), eh = (int)round(r[4] * scale);
    const int rw = max(ew - sw + 1, 1), rh = max(eh - sh + 1, 1);   // malformed -> 1 x 1
    const T bh = (T)rh / (T)PH, bw = (T)rw / (T)PW;
    const int hs = (int)floor((T)ph * bh), ws = (int)floor((T)pw * bw);
    const int he = (int)ceil((T)(ph + 1) * bh), we = (int)ceil((T)(pw + 1) * bw);
    q.hs = min(max(hs + sh, 0), H);
    q.he = min(max(he + sh, 0), H);
    q.ws = min(max(ws + sw, 0), W);
    q.we = min(max(we + sw, 0), W);
    return q;
}

// NHWC forward: one thread per (RoI, bin, channel vector), channel vector fastest.  Row-major scan with strict >: the first maximum wins, NaN never.
template <int VEC>
__global__ __launch_bounds__(256) void roi_pool_fwd_nhwc(const float* __restrict__ feat, const float* __restrict__ rois, int64_t total, int C, int H,
                                                          int W, float scale, int PH, int PW, float* __restrict__ out, int32_t* __restrict__ amax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cvecs = C / VEC, nbins = PH * PW;
    const int cv = (int)(i % cvecs), bin = (int)((i / cvecs) % nbins), n = (int)(i / cvecs / nbins);
    const PoolBin q = pool_bin<float>(rois + 5 * (size_t)n, scale, H, W, PH, PW, bin / PW, bin % PW);
    const bool empty = q.he <= q.hs || q.we <= q.ws;
    using V = typename VecT<VEC>::type;
    using I = typename VecT<VEC>::itype;
    V mv;
    I mi;
    float* m = reinterpret_cast<float*>(&mv);
    int* mx = reinterpret_cast<int*>(&mi);
#pragma unroll
    for (int j = 0; j < VEC; j++) { m[j] = empty ? 0.f : -FLT_MAX; mx[j] = -1; }
    const float* fb = feat + (size_t)q.b * H * W * C + (size_t)cv * VEC;
    for (int h = q.hs; h < q.he; h++)
        for (int w = q.ws; w < q.we; w++) {
            const int p = h * W + w;
            const V v = *reinterpret_cast<const V*>(fb + (size_t)p * C);
            const float* a = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if (a[j] > m[j]) { m[j] = a[j]; mx[j] = p; }
        }
    const size_t o = ((size_t)n * nbins + bin) * C + (size_t)cv * VEC;
    *reinterpret_cast<V*>(out + o) = mv;
    *reinterpret_cast<I*>(amax + o) = mi;
}

// NHWC backward: grad_feat[b, argmax, c] += grad.  One lane per CHANNEL: a wave's atomic instruction covers 64 consecutive channels of one bin,
// and the channels that share their argmax pixel form contiguous runs of it.  (16 B of channels per lane, as the forward reads, puts the lanes
// of each of its four atomic instructions 16 B apart: measured 3.1 ms against 1.3 ms at 2048 RoIs x 1024 channels.)
__global__ __launch_bounds__(256) void roi_pool_bwd_nhwc(const float* __restrict__ grad, const float* __restrict__ rois, const int32_t* __restrict__ amax,
                                                          int64_t total, int C, int H, int W, int nbins, float* __restrict__ gfeat) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), n = (int)(i / C / nbins);
    const int p = amax[i];
    if (p == -1) return;
    const int b = (int)rois[5 * (size_t)n];
    unsafeAtomicAdd(gfeat + ((size_t)b * H * W + p) * C + c, grad[i]);
}

// NCHW pair, T = float and double (AT_DISPATCH_FLOATING_TYPES, ROIPool_cuda.cu:134,177): the initial value is -FLT_MAX for both (:60)
template <typename T>
__global__ __launch_bounds__(256) void roi_pool_fwd_nchw(const T* __restrict__ feat, const T* __restrict__ rois, int64_t total, int C, int H, int W,
                                                          T scale, int PH, int PW, T* __restrict__ out, int32_t* __restrict__ amax) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pw = i % PW, ph = (i / PW) % PH, c = (i / PW / PH) % C, n = i / PW / PH / C;
        const PoolBin q = pool_bin<T>(rois + 5 * (size_t)n, scale, H, W, PH, PW, ph, pw);
        const bool empty = q.he <= q.hs || q.we <= q.ws;
        T m = empty ? (T)0 : (T)-FLT_MAX;
        int mx = -1;
        const T* plane = feat + ((size_t)q.b * C + c) * H * W;
        for (int h = q.hs; h < q.he; h++)
            for (int w = q.ws; w < q.we; w++) {
                const int p = h * W + w;
                if (plane[p] > m) { m = plane[p]; mx = p; }
            }
        out[i] = m;
        amax[i] = mx;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void roi_pool_bwd_nchw(const T* __restrict__ grad, const T* __restrict__ rois, const int32_t* __restrict__ amax,
                                                          int64_t total, int C, int H, int W, int nbins, T* __restrict__ gfeat) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (i / nbins) % C, n = i / nbins / C;
        const int p = amax[i];
        if (p == -1) continue;
        const int b = (int)rois[5 * (size_t)n];
        unsafeAtomicAdd(gfeat + ((size_t)b * C + c) * H * W + p, grad[i]);
    }
}

bool fits_i32(int64_t v) { return v >= 0 && v <= (int64_t)INT_MAX; }

template <typename T>
int pool_forward_nchw(const char* name, const T* feat, const T* rois, int K, int C, int H, int W, T scale, int PH, int PW, T* out, int32_t* amax,
                      hipStream_t st) {
    const int64_t total = (int64_t)K * C * PH * PW;
    roi_pool_fwd_nchw<T><<<(unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32), 256, 0, st>>>(feat, rois, total, C, H, W, scale, PH, PW, out, amax);
    ABR_CHECK_LAUNCH(name);
    return ABR_OK;
}

template <typename T>
int pool_backward_nchw(const char* name, const T* grad, const T* rois, const int32_t* amax, int K, int C, int H, int W, int PH, int PW, T* gfeat,
                       hipStream_t st) {
    const int64_t total = (int64_t)K * C * PH * PW;
    roi_pool_bwd_nchw<T><<<(unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32), 256, 0, st>>>(grad, rois, amax, total, C, H, W, PH * PW, gfeat);
    ABR_CHECK_LAUNCH(name);
    return ABR_OK;
}

#define POOL_SHAPE_CHECKS(name)                                                                                                    \
    ABR_REQUIRE(K >= 0 && B > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0, name ": bad shape");                               \
    ABR_REQUIRE(fits_i32((int64_t)K * C * PH * PW), name ": K*C*PH*PW = %lld does not fit int32", (long long)K * C * PH * PW);     \
    ABR_REQUIRE(fits_i32((int64_t)B * C * H * W), name ": the map's %lld elements do not fit int32", (long long)B * C * H * W)

// =====================================================================================================================================
// Deformable PS-RoI pooling (float32)
// =====================================================================================================================================
// Sample coordinates are computed in DOUBLE from the float32 operands, in the reference's order of operations.  A float32 coordinate near
// pixel 60 carries an error of a few 2^-18 pixels; through the bilinear slope that is up to 20 times the bound of the float32 sums that follow
// (tests/test_roi_pool_ref.py measures it), and it moves samples across the accept boundaries.  In double the accept decisions and the
// fractions are those of a float64 evaluation; the fractions and the four bilinear weights are formed in double and rounded once to float32
// (a weight (1 - dx)(1 - dy) formed from a rounded dx near 1 would be off by far more than its own size, and a map element may receive
// nothing but that weight's gradient); everything after them -- products, sums -- is float32.  A handful of double operations per sample, uniform across the wave's channels, beside 4 * VEC loads or 16 * VEC atomics.
struct PsRoi { int b; double x0, y0, rw, rh, bw, bh, sbw, sbh; };
struct PsBin { double ws, hs; int gh, gw, cell; };
struct PsTap {   // p12 = (y2, x1), p21 = (y1, x2): deform_pool_kernel_cuda.cu:45-48; ex = 1 - dx, ey = 1 - dy; w11 = ex ey, w12 = ex dy, w21 = dx ey, w22 = dx dy
    int p11, p12, p21, p22;
    float dx, dy, ex, ey, w11, w12, w21, w22;
};

#pragma clang fp contract(off)
__device__ __forceinline__ PsRoi ps_roi(const float* __restrict__ r, float scale, int P, int spp) {
    PsRoi g;
    const double s = (double)scale;
    g.b = (int)r[0];
    g.x0 = round((double)r[1]) * s - 0.5;
    g.y0 = round((double)r[2]) * s - 0.5;
    const double x1 = (round((double)r[3]) + 1.0) * s - 0.5, y1 = (round((double)r[4]) + 1.0) * s - 0.5;
    g.rw = fmax(x1 - g.x0, 0.1);
    g.rh = fmax(y1 - g.y0, 0.1);
    g.bw = g.rw / (double)P;
    g.bh = g.rh / (double)P;
    g.sbw = g.bw / (double)spp;
    g.sbh = g.bh / (double)spp;
    return g;
}

// the bin's sample origin (with the class's offset), its group cell and its part cell (:100-116).  The cells are the reference's fp32
// expressions, floor(float(ph) / P * part) and floor(float(ph) * G / P): the first is NOT always the exact integer ph * part / P (for
// P = part = 22 or 23 one bin lands a cell lower: tests/test_roi_pool_ref.py lists them); the min only keeps the index in range
#pragma clang fp contract(off)
__device__ __forceinline__ PsBin ps_bin(const PsRoi& g, const float* __restrict__ trans, int n, int cls, int ncls, int ph, int pw, int P, int part,
                                        int G, float tstd) {
    PsBin q;
    const int part_h = min((int)floorf((float)ph / (float)P * (float)part), part - 1);
    const int part_w = min((int)floorf((float)pw / (float)P * (float)part), part - 1);
    q.cell = part_h * part + part_w;
    double tx = 0.0, ty = 0.0;
    if (trans) {
        const float* t = trans + ((size_t)(n * ncls + cls) * 2) * part * part + q.cell;
        tx = (double)t[0] * (double)tstd;
        ty = (double)t[(size_t)part * part] * (double)tstd;
    }
    q.ws = (double)pw * g.bw + g.x0;
    q.ws = q.ws + tx * g.rw;
    q.hs = (double)ph * g.bh + g.y0;
    q.hs = q.hs + ty * g.rh;
    q.gw = min(max((int)floorf((float)pw * (float)G / (float)P), 0), G - 1);
    q.gh = min(max((int)floorf((float)ph * (float)G / (float)P), 0), G - 1);
    return q;
}

// one sample: false when it is skipped (both inequalities strict: a sample ON -0.5 or L - 0.5 is taken, then clamped) (:123-131)
#pragma clang fp contract(off)
__device__ __forceinline__ bool ps_tap(const PsRoi& g, const PsBin& q, int ih, int iw, int H, int W, PsTap* t) {
    double w = q.ws + (double)iw * g.sbw, h = q.hs + (double)ih * g.sbh;
    if (w < -0.5 || w > (double)W - 0.5 || h < -0.5 || h > (double)H - 0.5) return false;
    w = fmin(fmax(w, 0.0), (double)W - 1.0);
    h = fmin(fmax(h, 0.0), (double)H - 1.0);
    const double fx = floor(w), fy = floor(h);
    const int x1 = (int)fx, x2 = (int)ceil(w), y1 = (int)fy, y2 = (int)ceil(h);
    const double dx = w - fx, dy = h - fy, ex = 1.0 - dx, ey = 1.0 - dy;
    t->dx = (float)dx; t->dy = (float)dy; t->ex = (float)ex; t->ey = (float)ey;
    t->w11 = (float)(ex * ey); t->w12 = (float)(ex * dy); t->w21 = (float)(dx * ey); t->w22 = (float)(dx * dy);
    t->p11 = y1 * W + x1; t->p12 = y2 * W + x1; t->p21 = y1 * W + x2; t->p22 = y2 * W + x2;
    return true;
}

// One axis of a bin's sample grid, for the backward's separable form: the pixel range [lo, hi] its accepted samples touch (false: none
// accepted), and the weight they put on one pixel -- the same arithmetic as ps_tap, axis by axis.
#pragma clang fp contract(off)
__device__ __forceinline__ bool ps_axis_range(double start, double step, int spp, int L, int* lo, int* hi) {
    int a = L, b = -1;
    for (int i = 0; i < spp; i++) {
        double v = start + (double)i * step;
        if (v < -0.5 || v > (double)L - 0.5) continue;
        v = fmin(fmax(v, 0.0), (double)L - 1.0);
        a = min(a, (int)floor(v));
        b = max(b, (int)ceil(v));
    }
    *lo = a; *hi = b;
    return b >= a;
}

#pragma clang fp contract(off)
__device__ __forceinline__ double ps_axis_weight(double start, double step, int spp, int L, int pix) {
    double sum = 0.0;
    for (int i = 0; i < spp; i++) {
        double v = start + (double)i * step;
        if (v < -0.5 || v > (double)L - 0.5) continue;
        v = fmin(fmax(v, 0.0), (double)L - 1.0);
        const double f = floor(v), fr = v - f;
        if ((int)f == pix) sum += 1.0 - fr;
        if ((int)ceil(v) == pix) sum += fr;
    }
    return sum;
}

// the mask's sigmoid in double (one per bin, wave-uniform): what multiplies a value or a gradient is then rounded to float32 once
__device__ __forceinline__ double sigmoid_d(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

// Forward.  NHWC: one thread per (RoI, bin, output-channel vector), channels fastest; VEC = 4 needs group_size 1 (source channel == output
// channel), a class width and C that are multiples of 4.  NCHW: one thread per output, pw fastest.
#pragma clang fp contract(off)
template <int VEC, bool NHWC>
__global__ __launch_bounds__(256) void psroi_fwd(const float* __restrict__ feat, const float* __restrict__ rois, const float* __restrict__ trans,
                                                  const float* __restrict__ mlog, int64_t total, int C, int H, int W, float scale, int OD, int G, int P,
                                                  int part, int spp, float tstd, int ncls, int cec, float* __restrict__ out, float* __restrict__ cnt_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int PP = P * P, ov = OD / VEC;
    int cv, bin, n;
    if (NHWC) { cv = (int)(i % ov); bin = (int)((i / ov) % PP); n = (int)(i / ov / PP); }
    else { bin = (int)(i % PP); cv = (int)((i / PP) % OD); n = (int)(i / PP / OD); }
    const int ctop = cv * VEC, ph = bin / P, pw = bin % P;
    const PsRoi g = ps_roi(rois + 5 * (size_t)n, scale, P, spp);
    const PsBin q = ps_bin(g, trans, n, ctop / cec, ncls, ph, pw, P, part, G, tstd);
    const int c = (ctop * G + q.gh) * G + q.gw;
    const size_t HW = (size_t)H * W;
    const float* fb = NHWC ? feat + (size_t)g.b * HW * C + c : feat + ((size_t)g.b * C + c) * HW;
    const size_t sp = NHWC ? (size_t)C : 1;
    using V = typename VecT<VEC>::type;
    float sum[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) sum[j] = 0.f;
    int count = 0;
    for (int ih = 0; ih < spp; ih++)
        for (int iw = 0; iw < spp; iw++) {
            PsTap t;
            if (!ps_tap(g, q, ih, iw, H, W, &t)) continue;
            const V v11 = *reinterpret_cast<const V*>(fb + t.p11 * sp), v12 = *reinterpret_cast<const V*>(fb + t.p12 * sp);
            const V v21 = *reinterpret_cast<const V*>(fb + t.p21 * sp), v22 = *reinterpret_cast<const V*>(fb + t.p22 * sp);
            const float *a = reinterpret_cast<const float*>(&v11), *b = reinterpret_cast<const float*>(&v12);
            const float *cc = reinterpret_cast<const float*>(&v21), *d = reinterpret_cast<const float*>(&v22);
#pragma unroll
            for (int j = 0; j < VEC; j++) sum[j] += t.w11 * a[j] + t.w12 * b[j] + t.w21 * cc[j] + t.w22 * d[j];
            count++;
        }
    const float sig = mlog ? (float)sigmoid_d(mlog[(size_t)n * PP + bin]) : 1.f;
    V o, cn;
    float *op = reinterpret_cast<float*>(&o), *cp = reinterpret_cast<float*>(&cn);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const float raw = count == 0 ? 0.f : sum[j] / (float)count;
        op[j] = mlog ? raw * sig : raw;
        cp[j] = (float)count;
    }
    const size_t oi = NHWC ? ((size_t)n * PP + bin) * OD + ctop : (size_t)i;
    *reinterpret_cast<V*>(out + oi) = o;
    *reinterpret_cast<V*>(cnt_out + oi) = cn;
}

// Backward.  grid = K * part * part: workgroup (RoI n, part cell) owns grad_trans[n, :, :, cell] and grad_mask_logits of the cell's bins.
// It walks classes, then the cell's bins row-major, then its channels (strided over the threads), then the samples row-major; the
// per-thread partial sums meet in a fixed tree (block_sum) and thread 0 adds the results in that walk's order.
// One lane per channel (VEC = 1) in both layouts: every atomic instruction of a wave is then 256 contiguous bytes of one pixel in NHWC, the
// shape the float-atomic rate needs.  With 16 B per lane the four instructions' lanes sat 16 B apart: 83.6 ms against 21.4 ms at 2048 RoIs x
// 1024 channels, the latter at 94 % of the chip-wide float-atomic rate -- the floor of any form that adds every tap of every sample.
// So the map's gradient does not add every tap: a sample is accepted when its x AND its y are in range and its weights are products of an
// x-part and a y-part, hence a bin puts  dv * (sum of its y-weights on row y) * (sum of its x-weights on column x)  on pixel (y, x) -- one
// atomic per touched pixel (4 to 9 on a proposal-sized RoI) instead of 4 per sample (64 at sample_per_part 4), the weight sums in double.
#pragma clang fp contract(off)
template <bool NHWC>
__global__ __launch_bounds__(256) void psroi_bwd(const float* __restrict__ gout, const float* __restrict__ feat, const float* __restrict__ rois,
                                                  const float* __restrict__ trans, const float* __restrict__ mlog, const float* __restrict__ cnt_in,
                                                  int C, int H, int W, float scale, int OD, int G, int P, int part, int spp, float tstd, int ncls,
                                                  int cec, float* __restrict__ gfeat, float* __restrict__ gtrans, float* __restrict__ gmlog) {
    __shared__ float s_red[4];
    const int n = blockIdx.x / (part * part), cell = blockIdx.x % (part * part);
    const int PP = P * P;
    const size_t HW = (size_t)H * W;
    const PsRoi g = ps_roi(rois + 5 * (size_t)n, scale, P, spp);
    const size_t sp = NHWC ? (size_t)C : 1;
    const float rw = (float)g.rw, rh = (float)g.rh;
    const bool need_u = gtrans != nullptr || mlog != nullptr;
    constexpr int VEC = 1;
    using V = typename VecT<VEC>::type;
    for (int cls = 0; cls < ncls; cls++) {
        float* gt = gtrans ? gtrans + ((size_t)(n * ncls + cls) * 2) * part * part + cell : nullptr;
        if (gt && threadIdx.x == 0) { gt[0] = 0.f; gt[(size_t)part * part] = 0.f; }
        for (int bin = 0; bin < PP; bin++) {
            const int ph = bin / P, pw = bin % P;
            const PsBin q = ps_bin(g, trans, n, cls, ncls, ph, pw, P, part, G, tstd);
            if (q.cell != cell) continue;   // uniform
            const float lg = mlog ? mlog[(size_t)n * PP + bin] : 0.f;
            const double sig = mlog ? sigmoid_d(lg) : 1.0;
            float tdx = 0.f, tdy = 0.f, tm = 0.f;
            int y_lo, y_hi, x_lo, x_hi;
            const bool any_y = ps_axis_range(q.hs, g.sbh, spp, H, &y_lo, &y_hi), any_x = ps_axis_range(q.ws, g.sbw, spp, W, &x_lo, &x_hi);
            for (int ctop = cls * cec + (int)threadIdx.x * VEC; ctop < (cls + 1) * cec; ctop += 256 * VEC) {
                const size_t oi = NHWC ? ((size_t)n * PP + bin) * OD + ctop : ((size_t)n * OD + ctop) * PP + bin;
                const V gv = *reinterpret_cast<const V*>(gout + oi), cv = *reinterpret_cast<const V*>(cnt_in + oi);
                const float *go = reinterpret_cast<const float*>(&gv), *cn = reinterpret_cast<const float*>(&cv);
                if (cn[0] <= 0.f) continue;
                const int c = (ctop * G + q.gh) * G + q.gw;
                const size_t base = NHWC ? (size_t)g.b * HW * C + c : ((size_t)g.b * C + c) * HW;
                const float* fb = feat + base;
                float* gb = gfeat + base;
                float dv[VEC], raw[VEC];
#pragma unroll
                for (int j = 0; j < VEC; j++) { dv[j] = (float)((double)go[j] * sig / (double)cn[j]); raw[j] = 0.f; }   // g sigma / count: one rounding
                if (any_y && any_x)
                    for (int y = y_lo; y <= y_hi; y++) {
                        const double wy = ps_axis_weight(q.hs, g.sbh, spp, H, y);
                        if (wy == 0.0) continue;
                        for (int x = x_lo; x <= x_hi; x++) {
                            const double wx = ps_axis_weight(q.ws, g.sbw, spp, W, x);
                            if (wx == 0.0) continue;
                            const float wgt = (float)(wy * wx);
#pragma unroll
                            for (int j = 0; j < VEC; j++) unsafeAtomicAdd(gb + ((size_t)y * W + x) * sp + j, wgt * dv[j]);
                        }
                    }
                for (int ih = 0; need_u && ih < spp; ih++)     // the offset and mask-logit gradients need every sample's own taps
                    for (int iw = 0; iw < spp; iw++) {
                        PsTap t;
                        if (!ps_tap(g, q, ih, iw, H, W, &t)) continue;
                        const float q00 = t.w11, q01 = t.w12, q10 = t.w21, q11 = t.w22;
                        const V u00 = *reinterpret_cast<const V*>(fb + t.p11 * sp), u01 = *reinterpret_cast<const V*>(fb + t.p12 * sp);
                        const V u10 = *reinterpret_cast<const V*>(fb + t.p21 * sp), u11 = *reinterpret_cast<const V*>(fb + t.p22 * sp);
                        const float *U00 = reinterpret_cast<const float*>(&u00), *U01 = reinterpret_cast<const float*>(&u01);
                        const float *U10 = reinterpret_cast<const float*>(&u10), *U11 = reinterpret_cast<const float*>(&u11);
#pragma unroll
                        for (int j = 0; j < VEC; j++) {
                            if (gt) {   // :254-257
                                float ddx = (U11[j] * t.dy + U10[j] * t.ey - U01[j] * t.dy - U00[j] * t.ey) * tstd * dv[j];
                                ddx *= rw;
                                float ddy = (U11[j] * t.dx + U01[j] * t.ex - U10[j] * t.dx - U00[j] * t.ex) * tstd * dv[j];
                                ddy *= rh;
                                tdx += ddx;
                                tdy += ddy;
                            }
                            if (mlog) raw[j] += q00 * U00[j] + q01 * U01[j] + q10 * U10[j] + q11 * U11[j];
                        }
                    }
                if (mlog) {
#pragma unroll
                    for (int j = 0; j < VEC; j++) tm += go[j] * (raw[j] / cn[j]);
                }
            }
            if (gt) {
                const float sx = abr::block_sum<4>(tdx, s_red), sy = abr::block_sum<4>(tdy, s_red);
                if (threadIdx.x == 0) { gt[0] += sx; gt[(size_t)part * part] += sy; }
            }
            if (gmlog) {   // every class passes this bin once, in class order
                const float sm = abr::block_sum<4>(tm, s_red);
                if (threadIdx.x == 0) {
                    float* d = gmlog + (size_t)n * PP + bin;
                    const float v = (float)(sig * (1.0 - sig)) * sm;
                    *d = cls == 0 ? v : *d + v;
                }
            }
        }
    }
}

}  // namespace

// -------------------------------------------------------------------------------------------------------------------------------------
extern "C" int abr_roi_pool_forward(const float* feat, const float* rois, int K, int B, int C, int H, int W, float scale, int PH, int PW,
                                    int layout, float* out, int32_t* argmax, void* stream) {
    POOL_SHAPE_CHECKS("roi_pool_forward");
    ABR_REQUIRE(layout == ABR_NCHW || layout == ABR_NHWC, "roi_pool_forward: bad layout");
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(feat && rois && out && argmax, "roi_pool_forward: null pointer");
    hipStream_t st = abr::as_stream(stream);
    if (layout == ABR_NCHW) return pool_forward_nchw<float>("roi_pool_forward", feat, rois, K, C, H, W, scale, PH, PW, out, argmax, st);
    if (C % 4 == 0) {
        const int64_t total = (int64_t)K * PH * PW * (C / 4);
        roi_pool_fwd_nhwc<4><<<abr::cdiv(total, 256), 256, 0, st>>>(feat, rois, total, C, H, W, scale, PH, PW, out, argmax);
    } else {
        const int64_t total = (int64_t)K * PH * PW * C;
        roi_pool_fwd_nhwc<1><<<abr::cdiv(total, 256), 256, 0, st>>>(feat, rois, total, C, H, W, scale, PH, PW, out, argmax);
    }
    ABR_CHECK_LAUNCH("roi_pool_forward");
    return ABR_OK;
}

extern "C" int abr_roi_pool_backward(const float* grad, const float* rois, const int32_t* argmax, int K, int B, int C, int H, int W, int PH, int PW,
                                     int layout, int accumulate, float* gfeat, void* stream) {
    POOL_SHAPE_CHECKS("roi_pool_backward");
    ABR_REQUIRE(layout == ABR_NCHW || layout == ABR_NHWC, "roi_pool_backward: bad layout");
    ABR_REQUIRE(gfeat, "roi_pool_backward: null output");
    hipStream_t st = abr::as_stream(stream);
    if (!accumulate && hipMemsetAsync(gfeat, 0, sizeof(float) * (size_t)B * C * H * W, st) != hipSuccess) {
        abr::set_error("roi_pool_backward: memset failed");
        return ABR_E_LAUNCH;
    }
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(grad && rois && argmax, "roi_pool_backward: null pointer");
    if (layout == ABR_NCHW) return pool_backward_nchw<float>("roi_pool_backward", grad, rois, argmax, K, C, H, W, PH, PW, gfeat, st);
    const int64_t total = (int64_t)K * PH * PW * C;
    roi_pool_bwd_nhwc<<<abr::cdiv(total, 256), 256, 0, st>>>(grad, rois, argmax, total, C, H, W, PH * PW, gfeat);
    ABR_CHECK_LAUNCH("roi_pool_backward");
    return ABR_OK;
}

extern "C" int abr_roi_pool_forward_f64(const double* feat, const double* rois, int K, int B, int C, int H, int W, double scale, int PH, int PW,
                                        double* out, int32_t* argmax, void* stream) {
    POOL_SHAPE_CHECKS("roi_pool_forward_f64");
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(feat && rois && out && argmax, "roi_pool_forward_f64: null pointer");
    return pool_forward_nchw<double>("roi_pool_forward_f64", feat, rois, K, C, H, W, scale, PH, PW, out, argmax, abr::as_stream(stream));
}

extern "C" int abr_roi_pool_backward_f64(const double* grad, const double* rois, const int32_t* argmax, int K, int B, int C, int H, int W, int PH,
                                         int PW, double* gfeat, void* stream) {
    POOL_SHAPE_CHECKS("roi_pool_backward_f64");
    ABR_REQUIRE(gfeat, "roi_pool_backward_f64: null output");
    hipStream_t st = abr::as_stream(stream);
    if (hipMemsetAsync(gfeat, 0, sizeof(double) * (size_t)B * C * H * W, st) != hipSuccess) {   // at::zeros, ROIPool_cuda.cu:166
        abr::set_error("roi_pool_backward_f64: memset failed");
        return ABR_E_LAUNCH;
    }
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(grad && rois && argmax, "roi_pool_backward_f64: null pointer");
    return pool_backward_nchw<double>("roi_pool_backward_f64", grad, rois, argmax, K, C, H, W, PH, PW, gfeat, st);
}

#define PSROI_SHAPE_CHECKS(name)                                                                                                          \
    ABR_REQUIRE(K >= 0 && B > 0 && C > 0 && H > 0 && W > 0 && OD > 0 && G > 0 && P > 0 && part > 0 && spp > 0, name ": bad shape");       \
    ABR_REQUIRE(layout == ABR_NCHW || layout == ABR_NHWC, name ": bad layout");                                                           \
    ABR_REQUIRE((int64_t)OD * G * G <= C, name ": output_dim * group_size^2 = %lld exceeds the map's %d channels", (long long)OD * G * G, C); \
    ABR_REQUIRE(ncls >= 1 && OD % ncls == 0, name ": output_dim %d is not a multiple of the %d offset classes", OD, ncls);                \
    ABR_REQUIRE(fits_i32((int64_t)K * OD * P * P), name ": K*C*PH*PW = %lld does not fit int32", (long long)K * OD * P * P);              \
    ABR_REQUIRE(fits_i32((int64_t)B * C * H * W), name ": the map's %lld elements do not fit int32", (long long)B * C * H * W)

extern "C" int abr_deform_psroi_forward(const float* feat, const float* rois, const float* trans, const float* mask_logits, int K, int B, int C,
                                        int H, int W, float scale, int OD, int G, int P, int part, int spp, float trans_std, int num_classes,
                                        int layout, float* out, float* top_count, void* stream) {
    const int ncls = trans ? num_classes : 1;
    PSROI_SHAPE_CHECKS("deform_psroi_forward");
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(feat && rois && out && top_count, "deform_psroi_forward: null pointer");
    hipStream_t st = abr::as_stream(stream);
    const int cec = OD / ncls;
    if (layout == ABR_NCHW) {
        const int64_t total = (int64_t)K * OD * P * P;
        psroi_fwd<1, false><<<abr::cdiv(total, 256), 256, 0, st>>>(feat, rois, trans, mask_logits, total, C, H, W, scale, OD, G, P, part, spp, trans_std,
                                                                    ncls, cec, out, top_count);
    } else if (G == 1 && C % 4 == 0 && cec % 4 == 0) {
        const int64_t total = (int64_t)K * P * P * (OD / 4);
        psroi_fwd<4, true><<<abr::cdiv(total, 256), 256, 0, st>>>(feat, rois, trans, mask_logits, total, C, H, W, scale, OD, G, P, part, spp, trans_std,
                                                                   ncls, cec, out, top_count);
    } else {
        const int64_t total = (int64_t)K * P * P * OD;
        psroi_fwd<1, true><<<abr::cdiv(total, 256), 256, 0, st>>>(feat, rois, trans, mask_logits, total, C, H, W, scale, OD, G, P, part, spp, trans_std,
                                                                   ncls, cec, out, top_count);
    }
    ABR_CHECK_LAUNCH("deform_psroi_forward");
    return ABR_OK;
}

extern "C" int abr_deform_psroi_backward(const float* out_grad, const float* feat, const float* rois, const float* trans, const float* mask_logits,
                                         const float* top_count, int K, int B, int C, int H, int W, float scale, int OD, int G, int P, int part,
                                         int spp, float trans_std, int num_classes, int layout, float* grad_feat, float* grad_trans,
                                         float* grad_mask_logits, void* stream) {
    const int ncls = trans ? num_classes : 1;
    PSROI_SHAPE_CHECKS("deform_psroi_backward");
    ABR_REQUIRE((trans != nullptr) == (grad_trans != nullptr), "deform_psroi_backward: grad_trans goes with trans");
    ABR_REQUIRE((mask_logits != nullptr) == (grad_mask_logits != nullptr), "deform_psroi_backward: grad_mask_logits goes with mask_logits");
    ABR_REQUIRE((int64_t)K * part * part <= (int64_t)INT_MAX, "deform_psroi_backward: too many part cells");
    if (K == 0) return ABR_OK;
    ABR_REQUIRE(out_grad && feat && rois && top_count && grad_feat, "deform_psroi_backward: null pointer");
    hipStream_t st = abr::as_stream(stream);
    const int cec = OD / ncls;
    const unsigned grid = (unsigned)K * (unsigned)(part * part);
    if (layout == ABR_NCHW)
        psroi_bwd<false><<<grid, 256, 0, st>>>(out_grad, feat, rois, trans, mask_logits, top_count, C, H, W, scale, OD, G, P, part, spp, trans_std, ncls,
                                                   cec, grad_feat, grad_trans, grad_mask_logits);
    else
        psroi_bwd<true><<<grid, 256, 0, st>>>(out_grad, feat, rois, trans, mask_logits, top_count, C, H, W, scale, OD, G, P, part, spp, trans_std, ncls,
                                                  cec, grad_feat, grad_trans, grad_mask_logits);
    ABR_CHECK_LAUNCH("deform_psroi_backward");
    return ABR_OK;
}
