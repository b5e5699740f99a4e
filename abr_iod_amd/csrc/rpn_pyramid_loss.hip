// The RPN loss over a feature pyramid: both losses in ONE launch, the gradient of all levels in one memset + one launch.
//
// Reference: maskrcnn_benchmark/modeling/rpn/loss.py:104-148 with rpn/utils.py:10-45: per level a permute + reshape of both head outputs, a cat over
// the levels, the sampled indices gathered out of the concatenation, smooth_l1(beta = 1/9, sum) / #sampled and mean BCE-with-logits; autograd then
// scatters through the cat and the permutes into five dense tensors.  Here the fused head output of level l, NHWC [N, nloc_l, Cf] with the
// A logits in columns 0 .. A-1 and anchor a's deltas in columns A + 4a .. +3, already IS that order inside the level; what the concatenation adds is
// addressing.  With n = A * sum nloc_l and off_l = A * sum_{m<l} nloc_m, a sampled flat index g (the sampler's, offset by image * n) is
//
//     image i = g / n,  j = g % n,  level l: off_l <= j < off_{l+1},  location (j - off_l) / A,  anchor a = (j - off_l) % A.
//
// abr_rpn_pyramid_loss (one 1024-thread workgroup): slot s of the sampler's padded lists -- the N * max_pos positives, then the N * batch negatives,
//   -1 = padding -- is decoded, its logit read, and (positives) its four deltas; both sums go through a fixed tree: every thread adds its slots in
//   ascending order (s = t, t + 1024, ...), the waves xor-shuffle, wave 0 .. 15 are added in order.  No atomics, no scratch, no second workgroup:
//   the value depends on the inputs alone, not on the stream or on what else runs.  At most N * (max_pos + 4 max_pos + batch) values are read
//   (2 * 896 in training), so one workgroup is latency, not bandwidth.  Both losses are divided on the device by max(sum counts, 1).
//   With a gradient wanted it also leaves compact RECORDS: per slot the element offset of its logit in the gradient storage (-1: padding) and
//   (sigmoid(x) - y) / denom; per positive slot the offset of its first delta and the four smooth-L1 derivatives / denom.
// abr_rpn_pyramid_loss_backward: the gradient storage is ONE allocation, level l the [N, nloc_l, Cf] block at float offset Cf * N * sum_{m<l} nloc_m
//   (Cf % 4 == 0: every block 16-byte aligned).  One hipMemsetAsync over all of it, one scatter launch: record value times the upstream gradient of
//   its loss (two device scalars).  Sampled anchors are distinct and the logit and delta columns disjoint, so destinations are distinct: plain
//   stores; pad columns and unsampled anchors keep the memset's zero.
#include <algorithm>

#include "common.h"

namespace {

constexpr int MAXL = ABR_MAX_PYRAMID_LEVELS;
constexpr int TT = 1024;

struct LossLevels {          // by value in the kernel arguments: no device-side table
    const float* y[MAXL];    // [N, nloc, Cf] fused head output of the level
    int nloc[MAXL];
    int off[MAXL + 1];       // first anchor of the level in an image's concatenation; off[L] = n
    long long goff[MAXL];    // first float of the level's block in the gradient storage
};

__device__ __forceinline__ float sl1_ninth(float d, float* g) { return abr::sl1(d, 1.0f / 9, g); }   // the RPN's beta (rpn/loss.py:136)

// sum over the workgroup in a fixed order; valid in every thread
__device__ __forceinline__ float tree_sum(float v, float* sm) {
    v = abr::wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < TT / 64; w++) t += sm[w];
    return t;
}

__global__ __launch_bounds__(TT) void pyr_loss_kernel(LossLevels lv, int L, int N, int A, int Cf, const float* __restrict__ labels,
                                                      const float* __restrict__ reg_targets, const int64_t* __restrict__ pos, int n_pos,
                                                      const int64_t* __restrict__ neg, int n_neg, const int32_t* __restrict__ counts,
                                                      float* __restrict__ losses, int64_t* __restrict__ rec_dst, float* __restrict__ rec_val) {
    __shared__ float sm[TT / 64];
    const int n = lv.off[L], S = n_pos + n_neg;
    const long long total = (long long)N * n;
    int cnt = 0;
    for (int i = 0; i < 2 * N; i++) cnt += counts[i];
    const float inv = 1.f / fmaxf((float)cnt, 1.f);
    float obj = 0.f, box = 0.f;
    for (int s = threadIdx.x; s < S; s += TT) {
        const long long g = s < n_pos ? pos[s] : neg[s - n_pos];
        const bool live = g >= 0 && g < total;    // -1 pads a fixed-size list; an index outside the batch is never dereferenced
        long long d_obj = -1, d_reg = -1;
        float v_obj = 0.f;
        float4 v_reg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            const int i = (int)(g / n), j = (int)(g - (long long)i * n);
            int l = 0;
            while (l + 1 < L && j >= lv.off[l + 1]) l++;
            const int r = j - lv.off[l], loc = r / A, a = r - loc * A;
            const long long row = ((long long)i * lv.nloc[l] + loc) * Cf;
            const float* x = lv.y[l] + row;
            const float xv = x[a], yv = labels[g];
            obj += fmaxf(xv, 0.f) - xv * yv + log1pf(expf(-fabsf(xv)));        // (losses.hip's bce_gather_kernel)
            d_obj = lv.goff[l] + row + a;
            v_obj = (1.f / (1.f + expf(-xv)) - yv) * inv;
            if (s < n_pos) {
                const float* t = reg_targets + 4 * g;
                const float* dl = x + A + 4 * a;
                d_reg = lv.goff[l] + row + A + 4 * a;
                box += sl1_ninth(dl[0] - t[0], &v_reg.x);
                box += sl1_ninth(dl[1] - t[1], &v_reg.y);
                box += sl1_ninth(dl[2] - t[2], &v_reg.z);
                box += sl1_ninth(dl[3] - t[3], &v_reg.w);
                v_reg.x *= inv; v_reg.y *= inv; v_reg.z *= inv; v_reg.w *= inv;
            }
        }
        if (rec_dst) {
            rec_dst[s] = d_obj;
            rec_val[s] = v_obj;
            if (s < n_pos) {
                rec_dst[S + s] = d_reg;
                float* rv = rec_val + S + 4 * (size_t)s;
                rv[0] = v_reg.x; rv[1] = v_reg.y; rv[2] = v_reg.z; rv[3] = v_reg.w;
            }
        }
    }
    obj = tree_sum(obj, sm);
    box = tree_sum(box, sm);
    if (threadIdx.x == 0) {
        losses[0] = obj * inv;
        losses[1] = box * inv;
    }
}

__global__ __launch_bounds__(256) void pyr_loss_scatter_kernel(const int64_t* __restrict__ rec_dst, const float* __restrict__ rec_val, int S, int n_pos,
                                                               const float* __restrict__ g_obj, const float* __restrict__ g_box,
                                                               float* __restrict__ grad, long long grad_floats) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < S) {
        const long long d = rec_dst[t];
        if (d >= 0 && d < grad_floats) grad[d] = rec_val[t] * *g_obj;
    } else if (t < S + 4 * n_pos) {
        const int q = t - S;
        const long long d = rec_dst[S + (q >> 2)];
        if (d >= 0 && d + 3 < grad_floats) grad[d + (q & 3)] = rec_val[S + q] * *g_box;
    }
}

// the host tables -> the kernels' by-value argument; checks what both entries check.  *n_out = anchors per image, *grad_floats = the gradient storage
int fill_levels(const char* name, LossLevels& lv, const float* const* y, const int* nloc, int L, int N, int A, int Cf, bool need_y, int* n_out,
                long long* grad_floats) {
    ABR_REQUIRE(L >= 1 && L <= MAXL, "%s: L = %d levels, need 1 .. %d", name, L, MAXL);
    ABR_REQUIRE(N >= 0 && A >= 1, "%s: bad N or A", name);
    ABR_REQUIRE(Cf >= 5 * A, "%s: Cf = %d holds no 4A delta columns behind the A = %d logits", name, Cf, A);
    ABR_REQUIRE(Cf % 4 == 0, "%s: Cf = %d is not a multiple of 4 (the levels' gradient blocks would lose their 16-byte alignment)", name, Cf);
    ABR_REQUIRE(nloc && (!need_y || y), "%s: null level table", name);
    long long off = 0, goff = 0;
    for (int l = 0; l < MAXL; l++) {
        const int s = l < L ? l : 0;     // unused entries repeat level 0
        ABR_REQUIRE(nloc[s] >= 1, "%s: level %d: nloc = %d", name, s, nloc[s]);
        ABR_REQUIRE(!need_y || N == 0 || y[s], "%s: level %d: null pointer", name, s);
        lv.y[l] = need_y ? y[s] : nullptr;
        lv.nloc[l] = nloc[s];
        lv.off[l] = (int)off;
        lv.goff[l] = goff;
        if (l < L) {
            ABR_REQUIRE((long long)std::max(N, 1) * nloc[l] * Cf <= 0x7FFFFFFF, "%s: level %d does not fit int32", name, l);
            off += (long long)nloc[l] * A;
            goff += (long long)N * nloc[l] * Cf;
            ABR_REQUIRE(off <= 0x7FFFFFFF, "%s: the levels' anchors do not fit int32", name);
        }
    }
    for (int l = L; l <= MAXL; l++) lv.off[l] = (int)off;
    *n_out = (int)off;
    *grad_floats = goff;
    return ABR_OK;
}

}  // namespace

extern "C" int abr_rpn_pyramid_loss(const float* const* y_host, const int* nloc_host, int L, int N, int A, int Cf, const float* labels,
                                    const float* reg_targets, const int64_t* pos, int max_pos, const int64_t* neg, int batch, const int32_t* counts,
                                    float* losses, int64_t* rec_dst, float* rec_val, void* stream) {
    LossLevels lv;
    int n;
    long long gf;
    const int rc = fill_levels("rpn_pyramid_loss", lv, y_host, nloc_host, L, N, A, Cf, true, &n, &gf);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(max_pos >= 0 && batch >= 0 && N <= 4096 && (long long)N * ((long long)max_pos + batch) <= 0x0FFFFFFF,
                "rpn_pyramid_loss: bad max_pos / batch / N");
    ABR_REQUIRE(losses, "rpn_pyramid_loss: null pointer");
    ABR_REQUIRE((rec_dst == nullptr) == (rec_val == nullptr), "rpn_pyramid_loss: the two record arrays come together");
    const int n_pos = N * max_pos, n_neg = N * batch;
    hipStream_t st = abr::as_stream(stream);
    if (N == 0 || n_pos + n_neg == 0) {
        if (hipMemsetAsync(losses, 0, 2 * sizeof(float), st) != hipSuccess) {
            abr::set_error("rpn_pyramid_loss: memset failed");
            return ABR_E_LAUNCH;
        }
        return ABR_OK;
    }
    ABR_REQUIRE(labels && reg_targets && counts && (pos || !n_pos) && (neg || !n_neg), "rpn_pyramid_loss: null pointer");
    pyr_loss_kernel<<<1, TT, 0, st>>>(lv, L, N, A, Cf, labels, reg_targets, pos, n_pos, neg, n_neg, counts, losses, rec_dst, rec_val);
    ABR_CHECK_LAUNCH("rpn_pyramid_loss");
    return ABR_OK;
}

extern "C" int abr_rpn_pyramid_loss_backward(const int* nloc_host, int L, int N, int A, int Cf, const int64_t* rec_dst, const float* rec_val,
                                             int max_pos, int batch, const float* g_obj, const float* g_box, float* grad, void* stream) {
    LossLevels lv;
    int n;
    long long gf;
    const int rc = fill_levels("rpn_pyramid_loss_backward", lv, nullptr, nloc_host, L, N, A, Cf, false, &n, &gf);
    if (rc != ABR_OK) return rc;
    ABR_REQUIRE(max_pos >= 0 && batch >= 0 && (long long)N * ((long long)max_pos + batch) <= 0x0FFFFFFF, "rpn_pyramid_loss_backward: bad max_pos / batch");
    if (N == 0) return ABR_OK;
    ABR_REQUIRE(grad, "rpn_pyramid_loss_backward: null pointer");
    hipStream_t st = abr::as_stream(stream);
    if (hipMemsetAsync(grad, 0, (size_t)gf * sizeof(float), st) != hipSuccess) {
        abr::set_error("rpn_pyramid_loss_backward: memset failed");
        return ABR_E_LAUNCH;
    }
    const int n_pos = N * max_pos, S = n_pos + N * batch;
    if (S == 0) return ABR_OK;
    ABR_REQUIRE(rec_dst && rec_val && g_obj && g_box, "rpn_pyramid_loss_backward: null pointer");
    pyr_loss_scatter_kernel<<<abr::cdiv((int64_t)S + 4 * (int64_t)n_pos, 256), 256, 0, st>>>(rec_dst, rec_val, S, n_pos, g_obj, g_box, grad, gf);
    ABR_CHECK_LAUNCH("rpn_pyramid_loss_backward");
    return ABR_OK;
}
