// Device memory the library owns: the one statement of how it is allocated, zeroed, grown and refused ("Library-owned scratch").
// No HIP here: the policy is written against four backend operations, which common.hip binds to the HIP runtime and
// tests/host/scratch_main.cpp to a fake that can fail on demand.  A stream is an opaque pointer (nullptr = the null stream).
//
// Limits, as before the pool: the key is the stream handle alone (one process drives one device), and two host threads driving the SAME
// stream through the same slot are not supported (the second one's growth would free what the first one's kernels are about to use).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

namespace abr {

// one value per user of per-stream scratch
enum ScratchSlot {
    SCRATCH_WGRAD,          // conv_wgrad.hip: split-M partial tiles
    SCRATCH_WINO,           // Winograd V / M / U, one-off weight packs
    SCRATCH_SPLIT,          // conv_igemm.hip: split-K tickets + partial tiles
    SCRATCH_PREP_RING,      // conv_igemm.hip: the device half of the job ring
    SCRATCH_PREP_U,         // abr_conv_prepare_batch: fp32 Winograd-domain weights on their way to being packed
    SCRATCH_BIAS_TICKETS,   // abr_bias_grad: one ticket per column chunk
    SCRATCH_DET,            // det_ws: tickets + ring of partial sums (words: the two ring cursors)
    SCRATCH_TOPK,           // topk.hip (words: capacity in images, capacity in keys)
    SCRATCH_ROI_PYRAMID,    // roi_align.hip: the pyramid backward's float64 sums, every level's map back to back
    SCRATCH_RPN_PYRAMID,    // rpn_pyramid.hip: the pyramid ranking's histograms, counters, survivors, candidates and keys
    SCRATCH_RPN_SELECT,     // rpn_pyramid.hip: the cross-level selection's candidate words and thresholds
    SCRATCH_RETINA,         // retinanet.hip: histograms, counters, survivors, the segments' decoded rows and the bin lists
    SCRATCH_RETINA_TARGETS, // retinanet_loss.hip: the per-ground-truth maximum IoUs of abr_retina_targets
};
// process-wide zero-initialised words
enum WordSlot { WORDS_X6_FLAGS, WORDS_H3_STATS, WORDS_AMAX_RING, WORDS_SLOTS };

struct ScratchBackend {
    void* (*alloc)(size_t bytes);                            // nullptr = no memory
    void (*free)(void* p);
    bool (*sync)(void* stream);                              // returns once everything queued on `stream` has completed
    bool (*zero)(void* p, size_t bytes, void* stream);       // queued on `stream`
};

class ScratchPool {
    struct Entry { void* p = nullptr; size_t bytes = 0; uint64_t words[2] = {0, 0}; };

public:
    explicit ScratchPool(const ScratchBackend& be) : be_(be) {}
    ~ScratchPool() { release(); }
    ScratchPool(const ScratchPool&) = delete;
    ScratchPool& operator=(const ScratchPool&) = delete;

    // What a stateful user's callable is handed, valid under the pool's lock only.  words: two caller-owned words, zero at creation, kept
    // across growth and failure, never interpreted here.
    class Ref {
    public:
        uint64_t (&words)[2];
        // >= bytes of scratch for this (slot, stream).  A request that fits returns the same pointer and touches nothing.  One that does not:
        // synchronise the stream, free, allocate, zero the first zero_prefix bytes on the stream -- contents are not kept, *fresh says so.
        // nullptr: no memory or the fill failed; the entry is then empty, nothing is held, and a later call starts over.
        void* ensure(size_t bytes, size_t zero_prefix = 0, bool* fresh = nullptr) { return pool_.ensure(e_, stream_, bytes, zero_prefix, fresh); }

    private:
        friend class ScratchPool;
        Ref(ScratchPool& pool, Entry& e, void* stream) : words(e.words), pool_(pool), e_(e), stream_(stream) {}
        ScratchPool& pool_;
        Entry& e_;
        void* stream_;
    };

    // f(Ref) under the lock: one mutex, one map lookup.  f must not launch kernels.
    template <class F>
    auto locked(ScratchSlot slot, void* stream, F&& f) {
        std::lock_guard<std::mutex> g(mu_);
        return f(Ref(*this, entries_[std::make_pair((int)slot, stream)], stream));
    }
    // the stateless users' form of Ref::ensure
    void* scratch(ScratchSlot slot, void* stream, size_t bytes, size_t zero_prefix = 0) {
        return locked(slot, stream, [&](Ref r) { return r.ensure(bytes, zero_prefix); });
    }

    // `bytes` of process-wide words, allocated once.  Returns only after their zero fill has COMPLETED on the device, so no stream, blocking
    // or not, can see them unzeroed: one synchronous wait per slot per process.  nullptr: no memory (nothing held; a later call tries again).
    void* words(WordSlot slot, size_t bytes) {
        std::lock_guard<std::mutex> g(words_mu_);
        Entry& e = words_[slot];
        if (e.p) return e.p;
        void* p = be_.alloc(bytes);
        if (!p) return nullptr;
        if (!be_.zero(p, bytes, nullptr) || !be_.sync(nullptr)) { be_.free(p); return nullptr; }
        e.p = p;
        e.bytes = bytes;
        return p;
    }

    // bytes held, per-stream scratch and process words together
    int64_t bytes() {
        size_t n = 0;
        { std::lock_guard<std::mutex> g(mu_); for (auto& kv : entries_) n += kv.second.bytes; }
        { std::lock_guard<std::mutex> g(words_mu_); for (Entry& e : words_) n += e.bytes; }
        return (int64_t)n;
    }

    // frees everything (the caller knows the device is idle); the pool is usable again afterwards
    void release() {
        { std::lock_guard<std::mutex> g(mu_); for (auto& kv : entries_) drop(kv.second); entries_.clear(); }
        { std::lock_guard<std::mutex> g(words_mu_); for (Entry& e : words_) drop(e); }
    }

private:
    void drop(Entry& e) {
        if (e.p) be_.free(e.p);
        e.p = nullptr;
        e.bytes = 0;
    }
    void* ensure(Entry& e, void* stream, size_t bytes, size_t zero_prefix, bool* fresh) {
        if (fresh) *fresh = false;
        if (bytes <= e.bytes) return e.p;
        if (e.p) { (void)be_.sync(stream); drop(e); }   // the stream's queued kernels may still use the old buffer
        void* p = be_.alloc(bytes);
        if (!p) return nullptr;
        if (zero_prefix && !be_.zero(p, zero_prefix, stream)) { be_.free(p); return nullptr; }
        e.p = p;
        e.bytes = bytes;
        if (fresh) *fresh = true;
        return p;
    }

    const ScratchBackend be_;
    std::mutex mu_, words_mu_;
    std::map<std::pair<int, void*>, Entry> entries_;
    Entry words_[WORDS_SLOTS];
};

}  // namespace abr
