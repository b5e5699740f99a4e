// COCO run-length masks on the device (include/abr_iod_hip.h section 11): the codec pycocotools' mask_utils.decode / encode implement, restated
// from the format alone (nothing here was compared with pycocotools, which this project cannot run).
//   format   pixels in COLUMN-major order p = x * h + y; counts = lengths of alternating runs, the first of zeros; compressed: the i-th stored
//            value is counts[i] - counts[i-2] for i > 2 (counts[i] itself otherwise), written 5 bits a character, low bits first, bit 0x20 =
//            "more follows", bit 0x10 of the last character = sign, character = value + 48
//   decode   rle_scan_kernel, ONE workgroup per instance: token ends from the 0x20 bit -> block scan = token index -> the thread on a token's
//            last character assembles it -> two interleaved prefix sums (even / odd indices) undo the delta -> prefix sum = run ends.
//            rle_fill_*_kernel, the whole grid: every output pixel finds its run by a binary search of the run ends at its column-major
//            index and takes the run's parity; the packed words and the row-major bytes are written by mask_out.h's two loops.
//   encode   rle_colbits_kernel: the masks as bits in column-major order (a wave's ballot per 64 pixels); rle_runs_kernel, one workgroup per
//            instance: transitions = word ^ (word << 1 | previous word's top bit), popcount + block scan = compaction of the run starts, then
//            counts -> deltas -> characters per token -> block sum = the instance's bytes; rle_offsets_kernel: prefix sum over instances;
//            rle_emit_kernel, one workgroup per instance: the same scan again, now writing the characters.
// Everything is integer and bound by memory and scan latency; scans are wave-64 shuffles plus one LDS word per wave.  A workgroup only reads
// what ITS OWN threads wrote within a kernel (ordered by __syncthreads); hand-offs between workgroups are kernel boundaries.
// Safety: every index a kernel writes through is derived from the sizes the caller passed (never from the bytes being decoded), offsets are
// clamped into the buffers, and a malformed instance gives zeros and a totals[] that differs from h * w.
#include <algorithm>

#include "common.h"
#include "mask_out.h"

namespace {

constexpr int kScanThreads = 1024;
constexpr int kMaxTokenChars = 7;       // 35 bits: covers every difference of two counts below 2^31

typedef long long i64;

__device__ __forceinline__ i64 wave_scan_incl(i64 v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const i64 u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// inclusive scan over the workgroup's kScanThreads threads; `total` = the sum over all of them.  `sm`: 16 words, reusable after the call.
__device__ __forceinline__ i64 block_scan_incl(i64 v, i64* sm, i64& total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_scan_incl(v);
    __syncthreads();
    if (lane == 63) sm[wave] = v;
    __syncthreads();
    i64 before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kScanThreads / 64; i++) {
        const i64 s = sm[i];
        if (i < wave) before += s;
        all += s;
    }
    total = all;
    return v + before;
}

// ------------------------------------------------------------------------------------------------------------------------------- decode
// vals: int32 [n_items] workspace, item j of instance k at offsets[k] + j.  compressed: items are bytes -> stored values -> run ends, in place;
// else: items are the counts (`counts`), run ends written to vals.  nruns[k], totals[k]: see the header.
__global__ __launch_bounds__(kScanThreads) void rle_scan_kernel(const uint8_t* __restrict__ bytes, const int32_t* __restrict__ counts,
                                                                const i64* __restrict__ offsets, i64 n_items, i64 hw, int32_t* __restrict__ vals,
                                                                int32_t* __restrict__ nruns, i64* __restrict__ totals) {
    __shared__ i64 sm[16];
    __shared__ int s_err;
    const int k = blockIdx.x, tid = threadIdx.x;
    const i64 lo = abr::clamp64(offsets[k], 0, n_items), hi = abr::clamp64(offsets[k + 1], lo, n_items);
    const i64 len = hi - lo;
    int32_t* v = vals + lo;
    if (tid == 0) s_err = 0;
    __syncthreads();
    int err = 0;
    i64 ntok = len;
    if (bytes != nullptr) {
        const uint8_t* b = bytes + lo;
        i64 carry = 0;
        for (i64 base = 0; base < len; base += kScanThreads) {
            const i64 j = base + tid;
            int c = 0x20;                                   // (past the end: not a token end)
            if (j < len) {
                c = (int)b[j] - 48;
                if (c < 0 || c > 63) { err = max(err, 2); c = 0; }
            }
            const bool end = j < len && !(c & 0x20);
            i64 tot;
            const i64 incl = block_scan_incl(end ? 1 : 0, sm, tot);
            if (end) {
                // this token's characters: back to the previous token end, at most kMaxTokenChars
                int nch = 1;
                while (nch <= kMaxTokenChars && j - nch >= 0 && ((int)b[j - nch] - 48) >= 0 && ((int)b[j - nch] - 48) <= 63 && (((int)b[j - nch] - 48) & 0x20)) nch++;
                i64 x = 0;
                if (nch > kMaxTokenChars) err = max(err, 3);
                else {
                    for (int q = 0; q < nch; q++) x |= (i64)(((int)b[j - nch + 1 + q] - 48) & 0x1f) << (5 * q);
                    if (c & 0x10) x |= -((i64)1 << (5 * nch));
                    if (x < -(i64)0x7fffffff || x > (i64)0x7fffffff) { err = max(err, 3); x = 0; }
                }
                // (the token index is below the byte index: the slot was read, as a byte, in an earlier or this iteration -- bytes and vals are
                // different buffers, so nothing is overwritten before it is read)
                v[carry + incl - 1] = (int32_t)x;
            }
            carry += tot;
        }
        if (len > 0 && (((int)b[len - 1] - 48) & 0x20) && tid == 0) err = max(err, 1);      // the last token never ends
        ntok = carry;
        __syncthreads();
    }
    // stored values (or counts) -> counts -> run ends
    i64 ce = 0, co = 0, cs = 0;     // carries: even-index sum (from index 2), odd-index sum, run end
    for (i64 base = 0; base < ntok; base += kScanThreads) {
        const i64 i = base + tid;
        i64 cnt = 0;
        if (bytes != nullptr) {
            const i64 s = i < ntok ? (i64)v[i] : 0;
            i64 te, to;
            const i64 e = block_scan_incl((i >= 2 && !(i & 1)) ? s : 0, sm, te) + ce;
            const i64 o = block_scan_incl((i & 1) ? s : 0, sm, to) + co;
            ce += te;
            co += to;
            cnt = i == 0 ? s : ((i & 1) ? o : e);
        } else if (i < ntok) {
            cnt = (i64)counts[lo + i];
        }
        if (i < ntok && (cnt < 0 || cnt > (i64)0x7fffffff)) { err = max(err, 4); cnt = 0; }
        i64 ts;
        const i64 end = block_scan_incl(i < ntok ? cnt : 0, sm, ts) + cs;
        cs += ts;
        if (i < ntok) v[i] = (int32_t)min(end, (i64)0x7fffffff);
    }
    if (err) atomicMax(&s_err, err);
    __syncthreads();
    if (tid == 0) {
        const int e = s_err;
        nruns[k] = (int32_t)min(ntok, (i64)0x7fffffff);
        totals[k] = e ? -(i64)e : cs;
    }
}

// the value of pixel p: parity of the number of run ends <= p
__device__ __forceinline__ int rle_pixel(const int32_t* __restrict__ ends, int nr, int p) {
    int lo = 0, hi = nr;      // first index with ends[idx] > p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo & 1;
}

struct RleInst { const int32_t* ends; int nr; };
__device__ __forceinline__ RleInst rle_inst(const int32_t* vals, const i64* offsets, const int32_t* nruns, const i64* totals, i64 n_items, i64 hw, i64 k) {
    const i64 lo = abr::clamp64(offsets[k], 0, n_items), hi = abr::clamp64(offsets[k + 1], lo, n_items);
    RleInst r;
    r.ends = vals + lo;
    r.nr = totals[k] == hw ? (int)min((i64)nruns[k], hi - lo) : 0;      // malformed: no run ends, every pixel 0
    return r;
}

// the pixel predicate of the two fills (mask_out.h): the run ends of the instance, fetched once per instance, searched at x * h + y
struct RlePixel {
    const int32_t* vals;
    const i64* offsets;
    const int32_t* nruns;
    const i64* totals;
    i64 n_items, hw;
    int h;
    RleInst r;
    __device__ __forceinline__ void instance(i64 k) { r = rle_inst(vals, offsets, nruns, totals, n_items, hw, k); }
    __device__ __forceinline__ bool operator()(i64, int y, int x) const { return rle_pixel(r.ends, r.nr, x * h + y) != 0; }
};

__global__ __launch_bounds__(256) void rle_fill_u8_kernel(const int32_t* __restrict__ vals, const i64* __restrict__ offsets, const int32_t* __restrict__ nruns,
                                                          const i64* __restrict__ totals, i64 n_items, int h, int w, i64 numel, uint8_t* __restrict__ out) {
    abr::mask_write_u8(RlePixel{vals, offsets, nruns, totals, n_items, (i64)h * w, h, {nullptr, 0}}, numel, h, w, out);
}

__global__ __launch_bounds__(256) void rle_fill_bits_kernel(const int32_t* __restrict__ vals, const i64* __restrict__ offsets, const int32_t* __restrict__ nruns,
                                                            const i64* __restrict__ totals, i64 n_items, int h, int w, int Wq, i64 n_words,
                                                            unsigned long long* __restrict__ bits) {
    abr::mask_write_bits(RlePixel{vals, offsets, nruns, totals, n_items, (i64)h * w, h, {nullptr, 0}}, n_words, h, w, Wq, bits);
}

// ------------------------------------------------------------------------------------------------------------------------------- encode
// colbits [n, Cq] (Cq = ceil(h*w / 64)): bit p % 64 of word p / 64 = pixel p = x * h + y of the instance; tail bits zero
__global__ __launch_bounds__(256) void rle_colbits_kernel(const uint8_t* __restrict__ masks, const unsigned long long* __restrict__ packed, int h, int w,
                                                          int Wq, i64 Cq, i64 n_words, unsigned long long* __restrict__ colbits) {
    const int lane = threadIdx.x & 63;
    const i64 hw = (i64)h * w;
    const i64 n_waves = (i64)gridDim.x * 4;
    for (i64 wd = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); wd < n_words; wd += n_waves) {
        const i64 k = wd / Cq;
        const i64 p = (wd - k * Cq) * 64 + lane;
        bool set = false;
        if (p < hw) {
            const int x = (int)(p / h), y = (int)(p - (i64)x * h);
            if (masks != nullptr) set = masks[k * hw + (i64)y * w + x] == 1;
            else set = (packed[(k * h + y) * Wq + (x >> 6)] >> (x & 63)) & 1ull;
        }
        const unsigned long long word = __ballot(set);
        if (lane == 0) colbits[wd] = word;
    }
}

__device__ __forceinline__ int rle_token_chars(i64 x) {
    int n = 0;
    bool more = true;
    while (more) {
        const int c = (int)(x & 0x1f);
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        n++;
    }
    return n;
}

// starts: int32 [n, hw] workspace: the column-major positions where the value changes (the first counted against an implicit 0 before pixel 0)
// run i of an instance with nt transitions (nt + 1 runs): count(i) = T(i) - T(i-1), T(-1) = 0, T(nt) = hw
__device__ __forceinline__ i64 rle_count_at(const int32_t* T, i64 nt, i64 hw, i64 i) {
    if (i < 0) return 0;
    const i64 a = i >= nt ? hw : (i64)T[i];
    const i64 b = i == 0 ? 0 : (i64)T[i - 1];
    return a - b;
}
__device__ __forceinline__ i64 rle_stored_at(const int32_t* T, i64 nt, i64 hw, i64 i) {
    const i64 c = rle_count_at(T, nt, hw, i);
    return i > 2 ? c - rle_count_at(T, nt, hw, i - 2) : c;
}

__global__ __launch_bounds__(kScanThreads) void rle_runs_kernel(const unsigned long long* __restrict__ colbits, i64 Cq, i64 hw, int32_t* starts,
                                                                int32_t* __restrict__ nruns, i64* __restrict__ nbytes) {
    __shared__ i64 sm[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* cb = colbits + (i64)k * Cq;
    int32_t* T = starts + (i64)k * hw;
    i64 nt = 0;
    for (i64 base = 0; base < Cq; base += kScanThreads) {
        const i64 q = base + tid;
        unsigned long long tw = 0;
        if (q < Cq) {
            const unsigned long long wd = cb[q];
            const unsigned long long prev = q > 0 ? cb[q - 1] >> 63 : 0ull;
            tw = wd ^ ((wd << 1) | prev);
            const i64 left = hw - q * 64;                    // pixels in this word
            if (left < 64) tw &= (1ull << left) - 1ull;      // (the tail bits are zero pixels, not a transition)
        }
        i64 tot;
        i64 at = nt + block_scan_incl((i64)__popcll(tw), sm, tot) - __popcll(tw);
        while (tw) {                                         // at < hw: there are at most hw transitions
            const int bit = __ffsll((long long)tw) - 1;
            T[at++] = (int32_t)(q * 64 + bit);
            tw &= tw - 1ull;
        }
        nt += tot;
    }
    __syncthreads();                                         // T is complete for this workgroup's reads below
    i64 mine = 0;
    for (i64 i = tid; i <= nt; i += kScanThreads) mine += rle_token_chars(rle_stored_at(T, nt, hw, i));
    i64 tot;
    block_scan_incl(mine, sm, tot);
    if (tid == 0) {
        nruns[k] = (int32_t)(nt + 1);
        nbytes[k] = tot;
    }
}

__global__ __launch_bounds__(kScanThreads) void rle_offsets_kernel(const i64* __restrict__ nbytes, int n, i64* __restrict__ offsets) {
    __shared__ i64 sm[16];
    i64 carry = 0;
    if (threadIdx.x == 0) offsets[0] = 0;
    for (int base = 0; base < n; base += kScanThreads) {
        const int i = base + threadIdx.x;
        i64 tot;
        const i64 incl = block_scan_incl(i < n ? nbytes[i] : 0, sm, tot) + carry;
        if (i < n) offsets[i + 1] = incl;
        carry += tot;
    }
}

__global__ __launch_bounds__(kScanThreads) void rle_emit_kernel(const int32_t* __restrict__ starts, const int32_t* __restrict__ nruns,
                                                                const i64* __restrict__ offsets, int n, i64 hw, i64 capacity, uint8_t* __restrict__ out) {
    __shared__ i64 sm[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (offsets[n] > capacity) return;                       // all or nothing: the caller reads offsets[n] and comes back with room
    const int32_t* T = starts + (i64)k * hw;
    const i64 nt = abr::clamp64((i64)nruns[k] - 1, 0, hw);
    const i64 lo = offsets[k], hi = offsets[k + 1];
    i64 carry = lo;
    for (i64 base = 0; base <= nt; base += kScanThreads) {
        const i64 i = base + tid;
        i64 x = 0;
        int nch = 0;
        if (i <= nt) {
            x = rle_stored_at(T, nt, hw, i);
            nch = rle_token_chars(x);
        }
        i64 tot;
        i64 at = carry + block_scan_incl(nch, sm, tot) - nch;
        for (int q = 0; q < nch; q++) {
            int c = (int)(x & 0x1f);
            x >>= 5;
            if (q + 1 < nch) c |= 0x20;
            if (at >= lo && at < hi && at < capacity) out[at] = (uint8_t)(c + 48);
            at++;
        }
        carry += tot;
    }
}

bool image_ok(int h, int w) { return h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31); }

struct EncodeWs { size_t colbits, starts, nbytes, total; };
EncodeWs encode_ws(int n, int h, int w) {
    const size_t hw = (size_t)h * w, Cq = (hw + 63) / 64;
    EncodeWs e;
    e.colbits = 0;
    e.starts = e.colbits + (size_t)n * Cq * 8;
    e.nbytes = (e.starts + (size_t)n * hw * 4 + 7) / 8 * 8;
    e.total = e.nbytes + (size_t)n * 8;
    return e;
}

}  // namespace

extern "C" int64_t abr_rle_decode_workspace_bytes(int n, int64_t n_items) {
    if (n < 0 || n_items < 0) return -1;
    return (n_items + n) * 4;                                 // run ends per item + nruns per instance
}

extern "C" int abr_rle_decode(const uint8_t* bytes, const int32_t* counts, const int64_t* offsets, int n, int64_t n_items, int h, int w,
                              uint8_t* masks, uint64_t* bits, int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream) {
    ABR_REQUIRE(n >= 0 && n_items >= 0 && n_items < ((int64_t)1 << 31) && image_ok(h, w), "rle_decode: bad args (n, n_items >= 0, n_items < 2^31, 0 < h * w < 2^31)");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE((bytes != nullptr) != (counts != nullptr) || n_items == 0, "rle_decode: give the compressed bytes or the uncompressed counts, not both");
    ABR_REQUIRE(offsets && totals && (masks || bits), "rle_decode: null pointer (offsets, totals and at least one of masks / bits)");
    ABR_REQUIRE((reinterpret_cast<uintptr_t>(masks) & 3) == 0 && (reinterpret_cast<uintptr_t>(bits) & 7) == 0, "rle_decode: masks must be 4-byte aligned, bits 8-byte aligned");
    if (workspace_bytes < abr_rle_decode_workspace_bytes(n, n_items) || !workspace) {
        abr::set_error("rle_decode: workspace of %lld bytes, abr_rle_decode_workspace_bytes asks for %lld", (long long)workspace_bytes,
                       (long long)abr_rle_decode_workspace_bytes(n, n_items));
        return ABR_E_WORKSPACE;
    }
    hipStream_t st = abr::as_stream(stream);
    int32_t* vals = static_cast<int32_t*>(workspace);
    int32_t* nruns = vals + n_items;
    const i64* off = reinterpret_cast<const i64*>(offsets);
    i64* tot = reinterpret_cast<i64*>(totals);
    const int64_t hw = (int64_t)h * w;
    // (n_items == 0 with both pointers null: every instance is empty, which the scan reports as a total of 0)
    rle_scan_kernel<<<n, kScanThreads, 0, st>>>(counts ? nullptr : (bytes ? bytes : reinterpret_cast<const uint8_t*>(vals)), counts, off, n_items, hw, vals,
                                                nruns, tot);
    ABR_CHECK_LAUNCH("rle_decode (scan)");
    if (masks) {
        const int64_t numel = (int64_t)n * hw;
        rle_fill_u8_kernel<<<abr::quad_grid(numel), 256, 0, st>>>(vals, off, nruns, tot, n_items, h, w, numel, masks);
        ABR_CHECK_LAUNCH("rle_decode (fill)");
    }
    if (bits) {
        const int Wq = (w + 63) / 64;
        const int64_t n_words = (int64_t)n * h * Wq;
        rle_fill_bits_kernel<<<abr::wave_grid(n_words), 256, 0, st>>>(vals, off, nruns, tot, n_items, h, w, Wq, n_words, reinterpret_cast<unsigned long long*>(bits));
        ABR_CHECK_LAUNCH("rle_decode (fill bits)");
    }
    return ABR_OK;
}

extern "C" int64_t abr_rle_encode_workspace_bytes(int n, int h, int w) {
    if (n < 0 || !image_ok(h, w)) return -1;
    return (int64_t)encode_ws(n, h, w).total;
}

extern "C" int abr_rle_encode(const uint8_t* masks, const uint64_t* bits, int n, int h, int w, uint8_t* out_bytes, int64_t capacity, int64_t* offsets,
                              int32_t* nruns, void* workspace, int64_t workspace_bytes, void* stream) {
    ABR_REQUIRE(n >= 0 && image_ok(h, w) && capacity >= 0, "rle_encode: bad args (n, capacity >= 0, 0 < h * w < 2^31)");
    ABR_REQUIRE(offsets, "rle_encode: null offsets");
    hipStream_t st = abr::as_stream(stream);
    if (n == 0) {
        ABR_REQUIRE(hipMemsetAsync(offsets, 0, 8, st) == hipSuccess, "rle_encode: hipMemsetAsync failed");
        return ABR_OK;
    }
    ABR_REQUIRE((masks != nullptr) != (bits != nullptr), "rle_encode: give the uint8 masks or the packed words, not both");
    ABR_REQUIRE(nruns && (out_bytes || capacity == 0), "rle_encode: null pointer");
    if (workspace_bytes < abr_rle_encode_workspace_bytes(n, h, w) || !workspace) {
        abr::set_error("rle_encode: workspace of %lld bytes, abr_rle_encode_workspace_bytes asks for %lld", (long long)workspace_bytes,
                       (long long)abr_rle_encode_workspace_bytes(n, h, w));
        return ABR_E_WORKSPACE;
    }
    const EncodeWs e = encode_ws(n, h, w);
    char* ws = static_cast<char*>(workspace);
    auto* colbits = reinterpret_cast<unsigned long long*>(ws + e.colbits);
    auto* starts = reinterpret_cast<int32_t*>(ws + e.starts);
    auto* nbytes = reinterpret_cast<i64*>(ws + e.nbytes);
    const int64_t hw = (int64_t)h * w, Cq = (hw + 63) / 64;
    rle_colbits_kernel<<<abr::wave_grid(n * Cq), 256, 0, st>>>(masks, reinterpret_cast<const unsigned long long*>(bits), h, w, (w + 63) / 64, Cq, n * Cq, colbits);
    ABR_CHECK_LAUNCH("rle_encode (column-major bits)");
    rle_runs_kernel<<<n, kScanThreads, 0, st>>>(colbits, Cq, hw, starts, nruns, nbytes);
    ABR_CHECK_LAUNCH("rle_encode (runs)");
    rle_offsets_kernel<<<1, kScanThreads, 0, st>>>(nbytes, n, reinterpret_cast<i64*>(offsets));
    ABR_CHECK_LAUNCH("rle_encode (offsets)");
    rle_emit_kernel<<<n, kScanThreads, 0, st>>>(starts, nruns, reinterpret_cast<const i64*>(offsets), n, hw, capacity, out_bytes);
    ABR_CHECK_LAUNCH("rle_encode (emit)");
    return ABR_OK;
}
