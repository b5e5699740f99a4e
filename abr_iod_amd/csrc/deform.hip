// Deformable 3x3 convolution (DCNv1 / DCNv2, stride 1, pad 1, dilation 1) of the R-50-C4 body, NHWC fp32.
//
// The contraction is the library's 1x1 conv over a column tensor cols [B,H,W,9C] (tap k = 3i + j outermost, channel innermost: the OHWI
// weight [Cout][3][3][Cin] read as [Cout][9 Cin]); the two kernels here build those columns and take their gradient back to x and to the
// offset / mask field.  Semantics (modulated_deform_conv / deform_conv of maskrcnn_benchmark, restated):
//   om [B,H,W,Com]: for tap k and deformable group g (C / dg consecutive channels), dh = om[2k + 18g], dw = om[2k + 1 + 18g]; under v2
//   (modulated, dg == 1) m = sigmoid(om[18 + k]), else m = 1.
//   sample point h = ho - 1 + i + dh, w = wo - 1 + j + dw (fp32).  val = 0 unless -1 < h < H and -1 < w < W; else the bilinear
//   interpolation of the corners floor(h|w), floor(h|w) + 1, a corner outside the image contributing 0.  cols = m * val.
//   The gradient w.r.t. (dh, dw) is the derivative of that formula with the floors held fixed (zero outside the open box).
//
// Below them, the general form behind layers/dcn and _C.deform_conv_* / _C.modulated_deform_conv_* (abr_deform_im2col_general,
// abr_deform_col2im_coord_general; deform_conv_kernel_cuda.cu:198-460 and :578-780 restated, whose two bilinear helpers are the same function):
// any kernel of at most 49 taps, stride, padding, dilation, conv groups and deformable groups; offsets [B,Ho,Wo,dg*2K] and an optional
// mask [B,Ho,Wo,dg*K] that is used as given (no sigmoid); sample point h = ho*stride_h - pad_h + i*dil_h + dh; columns group-major
// [groups][B*Ho*Wo][K*C/groups].  The body's DCN keeps the two specialised kernels.
#include "common.h"

namespace {

struct Tap {
    bool in;                  // inside the open box -1 < h < H, -1 < w < W
    int hl, wl;               // floor(h), floor(w)
    float lh, lw, hh, hw;     // fractional parts and their complements
};

__device__ __forceinline__ Tap tap_at(float h, float w, int H, int W) {
    Tap t;
    t.in = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
    const float hf = floorf(h), wf = floorf(w);
    t.hl = t.in ? (int)hf : 0;
    t.wl = t.in ? (int)wf : 0;
    t.lh = h - hf; t.lw = w - wf;
    t.hh = 1.f - t.lh; t.hw = 1.f - t.lw;
    return t;
}

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

__device__ __forceinline__ float4 fma4(float a, float4 v, float4 acc) {
    acc.x = fmaf(a, v.x, acc.x); acc.y = fmaf(a, v.y, acc.y); acc.z = fmaf(a, v.z, acc.z); acc.w = fmaf(a, v.w, acc.w);
    return acc;
}

// One lane per (pixel, tap, 16 B channel group): lanes of one tap read 16 B of each corner pixel side by side and store 16 B of cols.
// total = B*H*W * 9 * C/4 < 2^31 (checked by the caller).
__global__ __launch_bounds__(256) void deform_im2col_kernel(const float* __restrict__ x, const float* __restrict__ om, int H, int W, int C, int Com,
                                                            int gs4, int modulated, float* __restrict__ cols, int total) {
    const int cv = C >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cg = i % cv;
    const int row = i / cv;               // pixel * 9 + tap
    const int k = row % 9, pix = row / 9;
    const int wo = pix % W, t = pix / W;
    const int ho = t % H, b = t / H;
    const int g = cg / gs4;
    const float* o = om + (int64_t)pix * Com;
    const float dh = o[2 * k + 18 * g], dw = o[2 * k + 1 + 18 * g];
    const float m = modulated ? sigmoid_f(o[18 + k]) : 1.f;
    const Tap p = tap_at((float)(ho - 1 + k / 3) + dh, (float)(wo - 1 + k % 3) + dw, H, W);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.in) {
        const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * H * W * cv + cg;
        const bool h0 = p.hl >= 0, h1 = p.hl + 1 <= H - 1, w0 = p.wl >= 0, w1 = p.wl + 1 <= W - 1;
        const int64_t q1 = ((int64_t)p.hl * W + p.wl) * cv, q3 = q1 + (int64_t)W * cv;
        if (h0 && w0) v = fma4(p.hh * p.hw, xb[q1], v);
        if (h0 && w1) v = fma4(p.hh * p.lw, xb[q1 + cv], v);
        if (h1 && w0) v = fma4(p.lh * p.hw, xb[q3], v);
        if (h1 && w1) v = fma4(p.lh * p.lw, xb[q3 + cv], v);
        v.x *= m; v.y *= m; v.z *= m; v.w *= m;
    }
    reinterpret_cast<float4*>(cols)[i] = v;
}

// One lane per (pixel, tap, fp32 channel); a workgroup holds 256 / C whole (pixel, tap) rows (C a power of two <= 256) or one row of C <= 1024
// lanes.  dx[corner] += m * w_corner * dcol: each wave instruction adds 64 consecutive channels (256 contiguous bytes) of one corner pixel.
// d_om: the per-lane terms of dh, dw (and the mask) are summed over the C / dg channels of a deformable group in a fixed order -- an xor
// butterfly inside the wave, then the waves' partials from LDS in wave order -- and written once: deterministic.  The padding channels
// [Com_real, Com) of d_om are written as 0.  amax (optional): max |d_om| into that amax word.
__global__ __launch_bounds__(1024) void deform_col2im_coord_kernel(const float* __restrict__ dcol, const float* __restrict__ x,
                                                                   const float* __restrict__ om, int H, int W, int C, int Com, int Com_real,
                                                                   int gs, int modulated, int rows, float* __restrict__ dx,
                                                                   float* __restrict__ dom, unsigned long long* amax, unsigned epoch) {
    __shared__ float red[16][3];
    const int rpb = blockDim.x / C;
    const int r_local = threadIdx.x / C, c = threadIdx.x % C;
    const int row = blockIdx.x * rpb + r_local;
    const bool live = row < rows;
    const int k = row % 9, pix = row / 9;
    const int g = c / gs;
    float sh = 0.f, sw = 0.f, sm = 0.f, m = 1.f, dm = 0.f;
    if (live) {
        const int wo = pix % W, t = pix / W;
        const int ho = t % H, b = t / H;
        const float* o = om + (int64_t)pix * Com;
        const float dh = o[2 * k + 18 * g], dw = o[2 * k + 1 + 18 * g];
        if (modulated) {   // m = 1 / (1 + e), dm/dz = m (1 - m) = e m^2 (no cancellation in 1 - m near m = 1)
            const float e = expf(-o[18 + k]);
            m = 1.f / (1.f + e);
            dm = e < INFINITY ? e * m * m : 0.f;
        }
        const Tap p = tap_at((float)(ho - 1 + k / 3) + dh, (float)(wo - 1 + k % 3) + dw, H, W);
        if (p.in) {
            const float gc = dcol[(int64_t)row * C + c];
            const int64_t base = (int64_t)b * H * W;
            const bool h0 = p.hl >= 0, h1 = p.hl + 1 <= H - 1, w0 = p.wl >= 0, w1 = p.wl + 1 <= W - 1;
            const int64_t q1 = (base + (int64_t)p.hl * W + p.wl) * C + c, q2 = q1 + C, q3 = q1 + (int64_t)W * C, q4 = q3 + C;
            const float v1 = h0 && w0 ? x[q1] : 0.f, v2 = h0 && w1 ? x[q2] : 0.f;
            const float v3 = h1 && w0 ? x[q3] : 0.f, v4 = h1 && w1 ? x[q4] : 0.f;
            const float gm = gc * m;
            if (h0 && w0) atomicAdd(dx + q1, gm * (p.hh * p.hw));
            if (h0 && w1) atomicAdd(dx + q2, gm * (p.hh * p.lw));
            if (h1 && w0) atomicAdd(dx + q3, gm * (p.lh * p.hw));
            if (h1 && w1) atomicAdd(dx + q4, gm * (p.lh * p.lw));
            sh = gm * (p.hw * (v3 - v1) + p.lw * (v4 - v2));
            sw = gm * (p.hh * (v2 - v1) + p.lh * (v4 - v3));
            if (modulated) sm = gc * (p.hh * p.hw * v1 + p.hh * p.lw * v2 + p.lh * p.hw * v3 + p.lh * p.lw * v4);
        }
    }
    // sum over the deformable group: lanes [g*gs, (g+1)*gs) of the row
    const int span = gs < 64 ? gs : 64;
    for (int off = span >> 1; off > 0; off >>= 1) {
        sh += __shfl_xor(sh, off, 64);
        sw += __shfl_xor(sw, off, 64);
        sm += __shfl_xor(sm, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if (gs > 64) {
        if ((threadIdx.x & 63) == 0) { red[wave][0] = sh; red[wave][1] = sw; red[wave][2] = sm; }
        __syncthreads();
        if (c % gs == 0) {
            sh = sw = sm = 0.f;
            for (int i = 0; i < gs / 64; i++) { sh += red[wave + i][0]; sw += red[wave + i][1]; sm += red[wave + i][2]; }
        }
    }
    unsigned am = 0;
    if (live) {
        float* d = dom + (int64_t)pix * Com;
        if (c % gs == 0) {
            d[2 * k + 18 * g] = sh;
            d[2 * k + 1 + 18 * g] = sw;
            am = max(__float_as_uint(sh) & 0x7FFFFFFFu, __float_as_uint(sw) & 0x7FFFFFFFu);
            if (modulated) {
                const float v = sm * dm;
                d[18 + k] = v;
                am = max(am, __float_as_uint(v) & 0x7FFFFFFFu);
            }
        }
        if (k == 0)
            for (int z = c; z < Com - Com_real; z += C) d[Com_real + z] = 0.f;
    }
    if (amax) abr::h3_amax_emit(amax, epoch, am);
}

// ---- the general deformable conv (any kernel, stride, padding, dilation, groups, deformable groups): abr_deform_*_general
struct Geom {
    int H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dlh, dlw;
    int K;       // kh * kw
    int rows;    // B * Ho * Wo
    int cg;      // C / groups: channels of one conv group
    int gs;      // C / dg: channels of one deformable group
    int dg;
};

// the sample point of output pixel (ho, wo) and tap k moved by (dh, dw): the integer part is exact, one fp32 add
__device__ __forceinline__ Tap tap_general(const Geom& q, int ho, int wo, int k, float dh, float dw) {
    return tap_at((float)(ho * q.sh - q.ph + (k / q.kw) * q.dlh) + dh, (float)(wo * q.sw - q.pw + (k % q.kw) * q.dlw) + dw, q.H, q.W);
}

// One lane per 16 B of cols [groups][rows][K * cg], in the order of the tensor: i = ((grp * rows + pix) * K + k) * cg / 4 + channel vector.
// The 4 channels of a lane lie in one conv group and one deformable group (cg % 4 == 0, gs % 4 == 0).  total < 2^31 (checked by the caller).
__global__ __launch_bounds__(256) void deform_im2col_general_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                                    const float* __restrict__ mask, Geom q, float* __restrict__ cols, int total) {
    const unsigned iu = blockIdx.x * 256u + threadIdx.x;      // (unsigned: the last workgroup may reach past 2^31)
    if (iu >= (unsigned)total) return;
    const int i = (int)iu;
    const int cgv = q.cg >> 2, cv = q.C >> 2;
    int r = i / cgv;
    const int cl = i - r * cgv;
    const int k = r % q.K;
    r /= q.K;
    const int pix = r % q.rows, grp = r / q.rows;
    const int c4 = grp * cgv + cl;              // channel vector of x
    const int g = (c4 << 2) / q.gs;
    const int wo = pix % q.Wo, t = pix / q.Wo;
    const int ho = t % q.Ho, b = t / q.Ho;
    const float* o = off + ((int64_t)pix * q.dg + g) * (2 * q.K) + 2 * k;
    const Tap p = tap_general(q, ho, wo, k, o[0], o[1]);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.in) {
        const int H = q.H, W = q.W;
        const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * H * W * cv + c4;
        const bool h0 = p.hl >= 0, h1 = p.hl + 1 <= H - 1, w0 = p.wl >= 0, w1 = p.wl + 1 <= W - 1;
        const int64_t q1 = ((int64_t)p.hl * W + p.wl) * cv, q3 = q1 + (int64_t)W * cv;
        if (h0 && w0) v = fma4(p.hh * p.hw, xb[q1], v);
        if (h0 && w1) v = fma4(p.hh * p.lw, xb[q1 + cv], v);
        if (h1 && w0) v = fma4(p.lh * p.hw, xb[q3], v);
        if (h1 && w1) v = fma4(p.lh * p.lw, xb[q3 + cv], v);
        if (mask) {
            const float m = mask[((int64_t)pix * q.dg + g) * q.K + k];
            v.x *= m; v.y *= m; v.z *= m; v.w *= m;
        }
    }
    reinterpret_cast<float4*>(cols)[i] = v;
}

// A unit is one (pixel, tap, deformable group): u = (pix * K + k) * dg + g, its gs channels consecutive in x.  `sub` lanes (a power of two:
// 64 when gs > 32, else the least one >= gs) serve a unit, 64 / sub units a wave; a lane walks the unit's channels sl, sl + sub, ...
// dx[corner] += m * w_corner * dcol: one wave instruction adds the min(gs, 64) consecutive channels of a unit at one corner pixel, and the
// units of a wave are consecutive groups of one (pixel, tap) -- 256 contiguous bytes when gs >= 64 or gs is a power of two with C >= 64.
// d_off / d_mask: each lane sums its channels in ascending order, then an xor butterfly over the unit's sub lanes; one lane writes.  Every
// element of d_off [rows][dg * 2K] and d_mask [rows][dg * K] has exactly one unit: all of both is written, in a fixed order (deterministic).
__global__ __launch_bounds__(256) void deform_col2im_coord_general_kernel(const float* __restrict__ dcol, const float* __restrict__ x,
                                                                          const float* __restrict__ off, const float* __restrict__ mask, Geom q,
                                                                          int sub, int units, float* __restrict__ dx, float* __restrict__ d_off,
                                                                          float* __restrict__ d_mask) {
    const int lane = threadIdx.x & 63;
    const int sl = lane & (sub - 1);
    const unsigned uu = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (64u / sub) + lane / sub;
    const bool live = uu < (unsigned)units;
    const int u = live ? (int)uu : 0;
    const int g = u % q.dg, r = u / q.dg;
    const int k = r % q.K, pix = r / q.K;
    float sh = 0.f, sw = 0.f, sm = 0.f;
    if (live) {
        const int wo = pix % q.Wo, t = pix / q.Wo;
        const int ho = t % q.Ho, b = t / q.Ho;
        const float* o = off + ((int64_t)pix * q.dg + g) * (2 * q.K) + 2 * k;
        const float m = mask ? mask[((int64_t)pix * q.dg + g) * q.K + k] : 1.f;
        const Tap p = tap_general(q, ho, wo, k, o[0], o[1]);
        if (p.in) {
            const int H = q.H, W = q.W, C = q.C;
            const bool h0 = p.hl >= 0, h1 = p.hl + 1 <= H - 1, w0 = p.wl >= 0, w1 = p.wl + 1 <= W - 1;
            const int64_t corner = ((int64_t)b * H * W + (int64_t)p.hl * W + p.wl) * C;
            for (int cl = sl; cl < q.gs; cl += sub) {
                const int c = g * q.gs + cl;
                const int grp = c / q.cg, cc = c - grp * q.cg;
                const float gc = dcol[((int64_t)grp * q.rows + pix) * ((int64_t)q.K * q.cg) + (int64_t)k * q.cg + cc];
                const int64_t q1 = corner + c, q2 = q1 + C, q3 = q1 + (int64_t)W * C, q4 = q3 + C;
                const float v1 = h0 && w0 ? x[q1] : 0.f, v2 = h0 && w1 ? x[q2] : 0.f;
                const float v3 = h1 && w0 ? x[q3] : 0.f, v4 = h1 && w1 ? x[q4] : 0.f;
                const float gm = gc * m;
                if (h0 && w0) atomicAdd(dx + q1, gm * (p.hh * p.hw));
                if (h0 && w1) atomicAdd(dx + q2, gm * (p.hh * p.lw));
                if (h1 && w0) atomicAdd(dx + q3, gm * (p.lh * p.hw));
                if (h1 && w1) atomicAdd(dx + q4, gm * (p.lh * p.lw));
                sh += gm * (p.hw * (v3 - v1) + p.lw * (v4 - v2));
                sw += gm * (p.hh * (v2 - v1) + p.lh * (v4 - v3));
                sm += gc * (p.hh * p.hw * v1 + p.hh * p.lw * v2 + p.lh * p.hw * v3 + p.lh * p.lw * v4);
            }
        }
    }
    for (int o = sub >> 1; o > 0; o >>= 1) {
        sh += __shfl_xor(sh, o, 64);
        sw += __shfl_xor(sw, o, 64);
        sm += __shfl_xor(sm, o, 64);
    }
    if (live && sl == 0) {
        float* d = d_off + ((int64_t)pix * q.dg + g) * (2 * q.K) + 2 * k;
        d[0] = sh;
        d[1] = sw;
        if (mask) d_mask[((int64_t)pix * q.dg + g) * q.K + k] = sm;
    }
}

// The argument checks both general entry points share: every one returns before any launch.
int general_geometry(const char* name, int B, int H, int W, int C, int Ho, int Wo, int kh, int kw, int stride_h, int stride_w, int pad_h,
                     int pad_w, int dil_h, int dil_w, int groups, int dg, Geom* q) {
    ABR_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: B, H, W, C must be positive, got %d, %d, %d, %d", name, B, H, W, C);
    ABR_REQUIRE(kh > 0 && kw > 0, "%s: kh, kw must be positive, got %d, %d", name, kh, kw);
    ABR_REQUIRE((int64_t)kh * kw <= 49, "%s: kh * kw = %lld exceeds 49", name, (long long)kh * kw);
    ABR_REQUIRE(stride_h > 0 && stride_w > 0, "%s: stride_h, stride_w must be positive, got %d, %d", name, stride_h, stride_w);
    ABR_REQUIRE(dil_h > 0 && dil_w > 0, "%s: dil_h, dil_w must be positive, got %d, %d", name, dil_h, dil_w);
    ABR_REQUIRE(pad_h >= 0 && pad_w >= 0, "%s: pad_h, pad_w must not be negative, got %d, %d", name, pad_h, pad_w);
    ABR_REQUIRE(groups > 0 && dg > 0, "%s: groups, dg must be positive, got %d, %d", name, groups, dg);
    ABR_REQUIRE(C % groups == 0, "%s: C = %d is not a multiple of groups = %d", name, C, groups);
    ABR_REQUIRE(C % dg == 0, "%s: C = %d is not a multiple of dg = %d", name, C, dg);
    ABR_REQUIRE((C / groups) % 4 == 0, "%s: C / groups = %d is not a multiple of 4", name, C / groups);
    ABR_REQUIRE((C / dg) % 4 == 0, "%s: C / dg = %d is not a multiple of 4", name, C / dg);
    const int64_t eh = (int64_t)H + 2 * (int64_t)pad_h - ((int64_t)dil_h * (kh - 1) + 1);
    const int64_t ew = (int64_t)W + 2 * (int64_t)pad_w - ((int64_t)dil_w * (kw - 1) + 1);
    ABR_REQUIRE(Ho > 0 && eh >= 0 && Ho == eh / stride_h + 1, "%s: Ho = %d does not follow from H, pad_h, dil_h, kh, stride_h", name, Ho);
    ABR_REQUIRE(Wo > 0 && ew >= 0 && Wo == ew / stride_w + 1, "%s: Wo = %d does not follow from W, pad_w, dil_w, kw, stride_w", name, Wo);
    const int64_t lanes = (int64_t)B * Ho * Wo * (kh * kw) * (C / 4);
    ABR_REQUIRE(lanes < ((int64_t)1 << 31), "%s: B * Ho * Wo * kh * kw * C / 4 = %lld is not below 2^31", name, (long long)lanes);
    ABR_REQUIRE((int64_t)B * H * W * C < ((int64_t)1 << 40), "%s: x is too large", name);
    *q = Geom{H, W, C, Ho, Wo, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, kh * kw, B * Ho * Wo, C / groups, C / dg, dg};
    return ABR_OK;
}

}  // namespace

extern "C" int abr_deform_im2col(const float* x, const float* om, int B, int H, int W, int C, int Com, int dg, int modulated, float* cols,
                                 void* stream) {
    ABR_REQUIRE(x && om && cols && B > 0 && H > 0 && W > 0 && C > 0 && dg > 0, "deform_im2col: bad args");
    ABR_REQUIRE(C % dg == 0 && (C / dg) % 4 == 0, "deform_im2col: C / deformable_groups must be a multiple of 4");
    ABR_REQUIRE(!modulated || dg == 1, "deform_im2col: the modulated form has one deformable group");
    ABR_REQUIRE(Com >= (modulated ? 27 : 18 * dg), "deform_im2col: the offset field has too few channels");
    const int64_t total = (int64_t)B * H * W * 9 * C;
    ABR_REQUIRE(total < (int64_t)0x7FFFFFF0, "deform_im2col: the column tensor must hold < 2^31 floats");
    const int lanes = (int)(total / 4);
    deform_im2col_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, abr::as_stream(stream)>>>(x, om, H, W, C, Com, C / dg / 4, modulated, cols,
                                                                                               lanes);
    ABR_CHECK_LAUNCH("deform_im2col");
    return ABR_OK;
}

extern "C" int abr_deform_col2im_coord(const float* dcol, const float* x, const float* om, int B, int H, int W, int C, int Com, int dg,
                                       int modulated, float* dx, float* d_om, uint64_t* d_om_amax, uint32_t d_om_amax_epoch, void* stream) {
    ABR_REQUIRE(dcol && x && om && dx && d_om && B > 0 && H > 0 && W > 0 && dg > 0, "deform_col2im_coord: bad args");
    ABR_REQUIRE(C >= 4 && C <= 1024 && (C & (C - 1)) == 0, "deform_col2im_coord: C must be a power of two in [4, 1024]");
    ABR_REQUIRE(C % dg == 0 && (C / dg) % 4 == 0, "deform_col2im_coord: C / deformable_groups must be a multiple of 4");
    ABR_REQUIRE(!modulated || dg == 1, "deform_col2im_coord: the modulated form has one deformable group");
    const int com_real = modulated ? 27 : 18 * dg;
    ABR_REQUIRE(Com >= com_real, "deform_col2im_coord: the offset field has too few channels");
    const int64_t total = (int64_t)B * H * W * 9 * C;
    ABR_REQUIRE(total < (int64_t)0x7FFFFFF0, "deform_col2im_coord: the column tensor must hold < 2^31 floats");
    const int rows = B * H * W * 9;
    const int threads = C < 256 ? 256 : C;
    const int rpb = threads / C;
    deform_col2im_coord_kernel<<<(unsigned)((rows + rpb - 1) / rpb), threads, 0, abr::as_stream(stream)>>>(
        dcol, x, om, H, W, C, Com, com_real, C / dg, modulated, rows, dx, d_om, reinterpret_cast<unsigned long long*>(d_om_amax), d_om_amax_epoch);
    ABR_CHECK_LAUNCH("deform_col2im_coord");
    return ABR_OK;
}

extern "C" int abr_deform_im2col_general(const float* x, const float* offset, const float* mask, int B, int H, int W, int C, int Ho, int Wo, int kh,
                                         int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int groups, int dg,
                                         float* cols, void* stream) {
    const char* name = "deform_im2col_general";
    Geom q;
    const int rc = general_geometry(name, B, H, W, C, Ho, Wo, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups, dg, &q);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(x && offset && cols, "%s: x, offset and cols must not be null", name);
    const int lanes = (int)((int64_t)q.rows * q.K * (C / 4));
    deform_im2col_general_kernel<<<abr::cdiv(lanes, 256), 256, 0, abr::as_stream(stream)>>>(x, offset, mask, q, cols, lanes);
    ABR_CHECK_LAUNCH(name);
    return ABR_OK;
}

extern "C" int abr_deform_col2im_coord_general(const float* dcol, const float* x, const float* offset, const float* mask, int B, int H, int W, int C,
                                               int Ho, int Wo, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                               int groups, int dg, float* dx, float* d_offset, float* d_mask, void* stream) {
    const char* name = "deform_col2im_coord_general";
    Geom q;
    const int rc = general_geometry(name, B, H, W, C, Ho, Wo, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups, dg, &q);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(dcol && x && offset && dx && d_offset, "%s: dcol, x, offset, dx and d_offset must not be null", name);
    ABR_REQUIRE((mask != nullptr) == (d_mask != nullptr), "%s: d_mask must be given exactly when mask is", name);
    int sub = 64;
    if (q.gs <= 32)
        for (sub = 4; sub < q.gs; sub <<= 1) {}
    const int64_t units = (int64_t)q.rows * q.K * dg;      // <= rows * K * C / 4 < 2^31
    const int per_block = 4 * (64 / sub);
    deform_col2im_coord_general_kernel<<<abr::cdiv(units, per_block), 256, 0, abr::as_stream(stream)>>>(dcol, x, offset, mask, q, sub, (int)units,
                                                                                                        dx, d_offset, d_mask);
    ABR_CHECK_LAUNCH(name);
    return ABR_OK;
}
