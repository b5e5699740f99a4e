// Drives the scratch policy of abr_iod_amd/csrc/scratch.h with a fake backend: one that counts live allocations, records every call in order
// and fails the n-th allocation or zero fill on demand.  Stand-alone (tests/test_scratch_host.py builds it with the address and undefined-
// behaviour sanitizers and runs it); exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "scratch.h"

namespace {

struct Call {
    char op;        // 's'ync, 'f'ree, 'a'lloc, 'z'ero
    void* stream;   // sync, zero
    void* p;        // free, alloc, zero
    size_t bytes;   // alloc, zero
};
std::mutex g_mu;   // the fake serves several threads
std::vector<Call> g_log;
std::map<void*, size_t> g_live;
int g_fail_alloc = 0, g_fail_zero = 0;   // n > 0: the n-th call from now fails

void* fake_alloc(size_t bytes) {
    std::lock_guard<std::mutex> g(g_mu);
    void* p = (g_fail_alloc && --g_fail_alloc == 0) ? nullptr : malloc(bytes);
    g_log.push_back({'a', nullptr, p, bytes});
    if (p) g_live[p] = bytes;
    return p;
}
void fake_free(void* p) {
    std::lock_guard<std::mutex> g(g_mu);
    g_log.push_back({'f', nullptr, p, 0});
    if (!g_live.erase(p)) { fprintf(stderr, "free of a pointer the fake does not hold\n"); abort(); }
    free(p);
}
bool fake_sync(void* stream) {
    std::lock_guard<std::mutex> g(g_mu);
    g_log.push_back({'s', stream, nullptr, 0});
    return true;
}
bool fake_zero(void* p, size_t bytes, void* stream) {
    std::lock_guard<std::mutex> g(g_mu);
    g_log.push_back({'z', stream, p, bytes});
    return !(g_fail_zero && --g_fail_zero == 0);
}
const abr::ScratchBackend kFake = {fake_alloc, fake_free, fake_sync, fake_zero};

size_t live_bytes() {
    std::lock_guard<std::mutex> g(g_mu);
    size_t n = 0;
    for (auto& kv : g_live) n += kv.second;
    return n;
}
std::string ops_since(size_t from) {
    std::lock_guard<std::mutex> g(g_mu);
    std::string s;
    for (size_t i = from; i < g_log.size(); i++) s += g_log[i].op;
    return s;
}
size_t log_size() {
    std::lock_guard<std::mutex> g(g_mu);
    return g_log.size();
}

int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                     \
        }                                                                   \
    } while (0)
// the accounting invariant, asserted after every step
#define CHECK_BYTES(pool) CHECK((size_t)(pool).bytes() == live_bytes())

void* stream(int i) { return reinterpret_cast<void*>((uintptr_t)0x1000 * (i + 1)); }

void test_fit_and_grow() {
    abr::ScratchPool pool(kFake);
    void* const s0 = stream(0);
    bool fresh = false;
    void* p = pool.locked(abr::SCRATCH_DET, s0, [&](abr::ScratchPool::Ref e) {
        CHECK(e.words[0] == 0 && e.words[1] == 0);   // zero at creation
        e.words[0] = 7;
        e.words[1] = 9;
        return e.ensure(1000, 100, &fresh);
    });
    CHECK(p && fresh);
    CHECK(ops_since(0) == "az");   // nothing to wait for or free the first time
    CHECK_BYTES(pool);

    // a fitting request: the same pointer, no backend call
    size_t mark = log_size();
    CHECK(pool.scratch(abr::SCRATCH_DET, s0, 1000, 100) == p);
    CHECK(pool.scratch(abr::SCRATCH_DET, s0, 1, 1) == p);
    pool.locked(abr::SCRATCH_DET, s0, [&](abr::ScratchPool::Ref e) { CHECK(e.ensure(500, 0, &fresh) == p && !fresh); return 0; });
    CHECK(log_size() == mark);
    CHECK_BYTES(pool);

    // a larger one: sync(stream), free(old), alloc, zero(prefix, stream) -- in that order, nothing else; words kept, fresh set
    void* q = pool.locked(abr::SCRATCH_DET, s0, [&](abr::ScratchPool::Ref e) { return e.ensure(5000, 128, &fresh); });
    CHECK(q && fresh);
    {
        std::lock_guard<std::mutex> g(g_mu);
        CHECK(g_log.size() == mark + 4);
        if (g_log.size() == mark + 4) {
            const Call *c = &g_log[mark];
            CHECK(c[0].op == 's' && c[0].stream == s0);
            CHECK(c[1].op == 'f' && c[1].p == p);
            CHECK(c[2].op == 'a' && c[2].p == q && c[2].bytes == 5000);
            CHECK(c[3].op == 'z' && c[3].p == q && c[3].bytes == 128 && c[3].stream == s0);
        }
    }
    pool.locked(abr::SCRATCH_DET, s0, [&](abr::ScratchPool::Ref e) { CHECK(e.words[0] == 7 && e.words[1] == 9); return 0; });
    CHECK_BYTES(pool);

    // no prefix, no fill
    mark = log_size();
    CHECK(pool.scratch(abr::SCRATCH_WGRAD, s0, 64) != nullptr);
    CHECK(ops_since(mark) == "a");
    CHECK_BYTES(pool);
}

void test_two_streams() {
    abr::ScratchPool pool(kFake);
    void *const s0 = stream(0), *const s1 = stream(1);
    void* a = pool.scratch(abr::SCRATCH_WINO, s0, 256, 16);
    void* b = pool.scratch(abr::SCRATCH_WINO, s1, 256, 16);
    void* c = pool.scratch(abr::SCRATCH_SPLIT, s0, 256, 16);   // another slot of the same stream is another buffer too
    CHECK(a && b && c && a != b && a != c && b != c);
    CHECK_BYTES(pool);
    const size_t mark = log_size();
    void* a2 = pool.scratch(abr::SCRATCH_WINO, s0, 4096, 16);
    CHECK(a2 != nullptr);
    {
        std::lock_guard<std::mutex> g(g_mu);
        for (size_t i = mark; i < g_log.size(); i++) CHECK(g_log[i].stream != s1 && g_log[i].p != b && g_log[i].p != c);
    }
    CHECK(ops_since(mark) == "sfaz");
    CHECK(pool.scratch(abr::SCRATCH_WINO, s1, 256, 16) == b);
    CHECK_BYTES(pool);
}

// the split_ws / prep_ring_take defect (an entry half-built by a failed allocation must not be handed out later) and the bias_grad leak
void test_failures() {
    abr::ScratchPool pool(kFake);
    void* const s0 = stream(0);
    for (int grown = 0; grown < 2; grown++) {   // from an empty entry, then from one that holds a buffer
        const size_t want = grown ? 8192 : 512, held_elsewhere = live_bytes();
        g_fail_alloc = 1;
        CHECK(pool.scratch(abr::SCRATCH_SPLIT, s0, want, 64) == nullptr);
        CHECK(live_bytes() == held_elsewhere - (grown ? 512 : 0));   // the entry holds nothing
        CHECK_BYTES(pool);
        size_t mark = log_size();
        void* p = pool.scratch(abr::SCRATCH_SPLIT, s0, want, 64);      // starts over: allocates, fills
        CHECK(p != nullptr);
        CHECK(ops_since(mark) == "az");
        CHECK_BYTES(pool);
        if (!grown) continue;

        g_fail_zero = 1;
        mark = log_size();
        CHECK(pool.scratch(abr::SCRATCH_SPLIT, s0, 2 * want, 64) == nullptr);
        CHECK(ops_since(mark) == "sfazf");   // the block whose fill failed went back
        CHECK(live_bytes() == 0);
        CHECK_BYTES(pool);
        CHECK(pool.scratch(abr::SCRATCH_SPLIT, s0, 2 * want, 64) != nullptr);
        CHECK(live_bytes() == 2 * want);
        CHECK_BYTES(pool);
    }
    // caller words outlive a failure
    pool.locked(abr::SCRATCH_TOPK, s0, [&](abr::ScratchPool::Ref e) { e.words[0] = 3; return e.ensure(64, 8); });
    g_fail_alloc = 1;
    CHECK(pool.scratch(abr::SCRATCH_TOPK, s0, 128, 8) == nullptr);
    pool.locked(abr::SCRATCH_TOPK, s0, [&](abr::ScratchPool::Ref e) { CHECK(e.words[0] == 3); return 0; });
    CHECK_BYTES(pool);
}

void test_words() {
    abr::ScratchPool pool(kFake);
    const size_t mark = log_size();
    void* got[2] = {nullptr, nullptr};
    std::thread t0([&] { got[0] = pool.words(abr::WORDS_H3_STATS, 2048); });
    std::thread t1([&] { got[1] = pool.words(abr::WORDS_H3_STATS, 2048); });
    t0.join();
    t1.join();
    CHECK(got[0] && got[0] == got[1]);
    {   // one allocation; the fill, then the wait for it -- both before either call returned
        std::lock_guard<std::mutex> g(g_mu);
        CHECK(g_log.size() == mark + 3);
        if (g_log.size() == mark + 3) {
            const Call* c = &g_log[mark];
            CHECK(c[0].op == 'a' && c[0].bytes == 2048);
            CHECK(c[1].op == 'z' && c[1].p == got[0] && c[1].bytes == 2048 && c[1].stream == nullptr);
            CHECK(c[2].op == 's' && c[2].stream == nullptr);
        }
    }
    CHECK_BYTES(pool);
    g_fail_zero = 1;
    CHECK(pool.words(abr::WORDS_X6_FLAGS, 4) == nullptr);
    CHECK(live_bytes() == 2048);
    CHECK_BYTES(pool);
    void* f = pool.words(abr::WORDS_X6_FLAGS, 4);
    CHECK(f && f != got[0] && pool.words(abr::WORDS_X6_FLAGS, 4) == f);
    CHECK(pool.scratch(abr::SCRATCH_DET, stream(0), 100, 10) != nullptr);
    CHECK((size_t)pool.bytes() == 2048 + 4 + 100);
    CHECK_BYTES(pool);
    pool.release();
    CHECK(live_bytes() == 0 && pool.bytes() == 0);
}

// eight threads look up their own streams' entries while one of them keeps growing its own: the sanitizers are the judge
void test_threads() {
    abr::ScratchPool pool(kFake);
    std::atomic<int> bad{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; t++)
        ts.emplace_back([&, t] {
            void* const st = stream(t);
            void* mine = pool.scratch(abr::SCRATCH_WINO, st, 64, 8);
            for (int i = 0; i < 2000; i++) {
                if (t == 0) {
                    char* p = static_cast<char*>(pool.scratch(abr::SCRATCH_WINO, st, 64 + (size_t)i, 8));
                    if (!p) bad++; else p[64 + i - 1] = 1;   // the whole of the grown buffer is this thread's
                } else {
                    char* p = static_cast<char*>(pool.scratch(abr::SCRATCH_WINO, st, 64, 8));
                    if (p != mine) bad++; else p[i & 63] = (char)t;
                    const bool ok = pool.locked(abr::SCRATCH_DET, st, [&](abr::ScratchPool::Ref e) { return e.ensure(32, 4) && e.words[0]++ == (uint64_t)i; });
                    if (!ok) bad++;
                }
                if ((i & 255) == 0) (void)pool.bytes();
            }
        });
    for (auto& t : ts) t.join();
    CHECK(bad == 0);
    CHECK_BYTES(pool);
}

}  // namespace

int main() {
    test_fit_and_grow();
    CHECK(live_bytes() == 0);   // every pool above released what it held when it went away
    test_two_streams();
    test_failures();
    test_words();
    test_threads();
    CHECK(live_bytes() == 0);
    if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    printf("scratch ok\n");
    return 0;
}
