// Stand-alone check of the memory owners of csrc/hobbit_mem.hpp (Buf, GrowBuf, Pool, Pooled) against a counting fake in place of HIP: the
// header is compiled as it is, with HOBBIT_MEM_FAKE defined and the seam mem::raw supplied here.  The fake hands out made-up addresses (nothing
// is really allocated, so sizes of GiB cost nothing), keeps its own table of what is live, aborts on a free of something it does not hold, records
// the order of its calls ('A'lloc, 'F'ree, 'W'ait) and can be told to fail chosen allocations.  After every step the header's own live counter
// must agree with the fake's table.  Exit status 0 and "ok" when every check holds; the first failed check prints its line and exits with 1.
// tests/test_mem_owners_cpu.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>

namespace hobbit { namespace mem { namespace raw {
using stream_t = void *;
static std::map<void *, size_t> held;          // the fake's bookkeeping: address -> bytes
static size_t held_bytes = 0, next_addr = 0, allocs = 0;
static std::string order;                      // 'A', 'F', 'W' in call order
static long fail_at = -1; static int fail_n = 0;     // the allocations number fail_at .. fail_at + fail_n - 1 (counted from `allocs`) fail
static void *alloc(int, size_t bytes, unsigned) {
    order += 'A';
    const long k = (long)allocs++;
    if (fail_at >= 0 && k >= fail_at && k < fail_at + fail_n) return nullptr;
    void *p = reinterpret_cast<void *>((++next_addr) << 12);
    held[p] = bytes; held_bytes += bytes;
    return p;
}
static void free(int, void *p) {
    order += 'F';
    auto it = held.find(p);
    if (it == held.end()) { fprintf(stderr, "fake: free of %p, which is not live (double free?)\n", p); exit(1); }
    held_bytes -= it->second; held.erase(it);
}
static void wait(stream_t) { order += 'W'; }
}}}

#define HOBBIT_MEM_FAKE
#include "hobbit_mem.hpp"

using namespace hobbit::mem;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "mem_owner_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)
// the header's counter against the fake's table
#define AGREE() do { CHECK(live_allocs.load() == raw::held.size()); CHECK(live_bytes.load() == raw::held_bytes); } while (0)
static void fail_from(long k, int n) { raw::fail_at = k < 0 ? -1 : (long)raw::allocs + k; raw::fail_n = n; }
static size_t live() { AGREE(); return raw::held.size(); }

static void test_buf() {
    raw::order.clear();
    {
        Buf<uint64_t> a; Buf<uint8_t, Pinned> h;
        CHECK(!a && a.bytes() == 0);
        CHECK(a.alloc(100) == 0 && a && a.bytes() == 800); AGREE();
        CHECK(h.alloc(7) == 0 && h.bytes() == 7); CHECK(live() == 2);
        uint64_t *raw_a = a;
        Buf<uint64_t> b(std::move(a));                          // moved-from: empty, frees nothing
        CHECK(!a && a.bytes() == 0 && b.get() == raw_a && b.bytes() == 800); CHECK(live() == 2);
        Buf<uint64_t> c; CHECK(c.alloc(1) == 0); CHECK(live() == 3);
        c = std::move(b);                                       // move assignment frees what the target held, once
        CHECK(!b && c.get() == raw_a); CHECK(live() == 2);
        uint64_t *out = c.release();                            // hand over without freeing
        CHECK(out == raw_a && !c && c.bytes() == 0); CHECK(live() == 2);
        Buf<uint64_t> d; d.adopt(out, 800);                     // and back, without allocating
        CHECK(d.get() == raw_a && d.bytes() == 800); CHECK(live() == 2);
        CHECK(d.alloc(3) == 0 && d.bytes() == 24); CHECK(live() == 2);      // alloc drops what it held
        d.reset(); d.reset(); CHECK(live() == 1);
    }
    CHECK(live() == 0);
    CHECK(raw::order == "AAAFFAFF");                            // no wait anywhere: a Buf never synchronises
    fail_from(0, 1);
    Buf<int> f; CHECK(f.alloc(4) == HOBBIT_ENOMEM && !f && f.bytes() == 0); CHECK(live() == 0);
    fail_from(-1, 0);
}

static void test_grow() {
    GrowBuf<Device> g; void *p = nullptr, *q = nullptr;
    raw::order.clear();
    CHECK(g.ensure(nullptr, 1000, &p) == 0 && p && g.bytes() == 1000);
    CHECK(raw::order == "A");                                   // nothing to wait for or free the first time
    raw::order.clear();
    CHECK(g.ensure(nullptr, 1000, &q) == 0 && q == p); CHECK(g.ensure(nullptr, 1, &q) == 0 && q == p);
    CHECK(raw::order.empty());                                  // not above the capacity: no raw call
    CHECK(g.ensure(nullptr, 1001, &q) == 0 && g.bytes() == 1001);
    CHECK(raw::order == "WFA");                                 // wait, free, allocate -- in that order
    CHECK(live() == 1);
    fail_from(0, 1);
    CHECK(g.ensure(nullptr, 5000, &q) == HOBBIT_ENOMEM && g.bytes() == 0); CHECK(live() == 0);
    fail_from(-1, 0);
    CHECK(g.ensure(nullptr, 10, &q) == 0); CHECK(live() == 1);
}

static void test_pool() {
    {
        Pool pool; void *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(pool.get(4096, &a) == 0); CHECK(live() == 1);
        pool.put(4096, a); CHECK(pool.parked() == 1 && pool.parked_bytes() == 4096); CHECK(live() == 1);
        raw::order.clear();
        CHECK(pool.get(4096, &b) == 0 && b == a && raw::order.empty());       // same size: the same pointer, no raw call, no wait
        CHECK(pool.parked() == 0 && pool.parked_bytes() == 0);
        pool.put(4096, b);
        CHECK(pool.get(4097, &c) == 0 && c != a && raw::order == "A");        // exact size only: another size allocates
        CHECK(pool.parked() == 1); CHECK(live() == 2);
        pool.put(4097, c); pool.put(1, nullptr); CHECK(pool.parked() == 2);
        raw::order.clear();
        pool.drain(); CHECK(raw::order == "WFF" && pool.parked() == 0 && pool.parked_bytes() == 0); CHECK(live() == 0);
        raw::order.clear(); pool.drain(); CHECK(raw::order.empty());          // nothing parked: not even a wait
    }
    {   // at most 48 parked: the 49th is freed (after a wait), not parked
        Pool pool; void *p[49];
        for (auto &q : p) CHECK(pool.get(64, &q) == 0);
        for (int i = 0; i < 48; i++) pool.put(64, p[i]);
        CHECK(pool.parked() == Pool::MAX_PARKED); CHECK(live() == 49);
        raw::order.clear();
        pool.put(64, p[48]); CHECK(raw::order == "WF" && pool.parked() == 48); CHECK(live() == 48);
    }
    CHECK(live() == 0);                                                       // ~Pool frees what is still parked
    {   // at most 8 GiB parked
        Pool pool; void *a, *b, *c; const size_t G = (size_t)1 << 30;
        CHECK(pool.get(5 * G, &a) == 0 && pool.get(3 * G, &b) == 0 && pool.get(1, &c) == 0);
        pool.put(5 * G, a); pool.put(3 * G, b); CHECK(pool.parked() == 2 && pool.parked_bytes() == Pool::MAX_BYTES);     // exactly 8 GiB still parks
        raw::order.clear();
        pool.put(1, c); CHECK(raw::order == "WF" && pool.parked() == 2); CHECK(live() == 2);
    }
    CHECK(live() == 0);
    {   // a failed allocation drains the pool and tries once more
        Pool pool; void *a, *b = nullptr;
        CHECK(pool.get(100, &a) == 0); pool.put(100, a);
        raw::order.clear(); fail_from(0, 1);
        CHECK(pool.get(200, &b) == 0 && b); CHECK(raw::order == "AWFA" && pool.parked() == 0); CHECK(live() == 1);
        pool.put(200, b);
        raw::order.clear(); fail_from(0, 2);                                  // twice: HOBBIT_ENOMEM and a null pointer
        void *c = &pool;
        CHECK(pool.get(300, &c) == HOBBIT_ENOMEM && c == nullptr); CHECK(raw::order == "AWFA"); CHECK(live() == 0);
        fail_from(-1, 0);
    }
    {   // the raw pointers of hobbit_malloc / hobbit_free
        Pool pool; void *a = nullptr; int other;
        CHECK(pool.lend(500, &a) == 0 && a); CHECK(!pool.take_back(&other));
        CHECK(pool.take_back(a) && pool.parked() == 1 && pool.parked_bytes() == 500); CHECK(!pool.take_back(a));
    }
    CHECK(live() == 0);
    {   // the pooled owner goes back to its pool, once
        Pool pool;
        {
            Pooled<uint32_t> x, y;
            CHECK(x.get(pool, 256) == 0 && x && x.bytes() == 256);
            uint32_t *px = x;
            y = std::move(x); CHECK(!x && y.get() == px); CHECK(live() == 1 && pool.parked() == 0);
            Pooled<uint32_t> z(std::move(y)); CHECK(!y && z.get() == px);
        }
        CHECK(pool.parked() == 1 && pool.parked_bytes() == 256); CHECK(live() == 1);
        Pooled<uint32_t> w; raw::order.clear(); CHECK(w.get(pool, 256) == 0 && raw::order.empty() && pool.parked() == 0);
        w.reset(); w.reset(); CHECK(pool.parked() == 1);
    }
    CHECK(live() == 0);
}

// The shape of every *_begin of the library: the handle in a unique_ptr takes N pooled buffers (steps 0 .. N-1) and then makes a fallible call
// (step N); *out gets the handle on the last line only.  Step k fails -- an allocation together with the pool's retry.
struct Handle5 { static constexpr int N = 5; Pooled<uint8_t> b[N]; };
static int begin(Pool &pool, bool call_fails, Handle5 **out) {
    std::unique_ptr<Handle5> h(new Handle5());
    for (int i = 0; i < Handle5::N; i++) if (h->b[i].get(pool, 1000 + 10 * (i % 2))) return HOBBIT_ENOMEM;
    if (call_fails) return HOBBIT_EHIP;
    *out = h.release();
    return 0;
}
static void test_begin() {
    const int N = Handle5::N;
    for (int k = 0; k <= N; k++) {
        Pool pool; Handle5 *h = nullptr;
        if (k < N) fail_from(k, 2);
        const int rc = begin(pool, k == N, &h);
        fail_from(-1, 0);
        CHECK(rc == (k < N ? HOBBIT_ENOMEM : HOBBIT_EHIP) && h == nullptr);
        CHECK(live() == pool.parked());                          // what was taken went back to the pool (or was freed by the retry's drain) ...
        pool.drain();
        CHECK(live() == 0);                                      // ... and nothing else survived the error return
    }
    Pool pool; Handle5 *h = nullptr;
    CHECK(begin(pool, false, &h) == 0 && h); CHECK(live() == (size_t)N && pool.parked() == 0);
    delete h; CHECK(live() == (size_t)N && pool.parked() == (size_t)N);
    raw::order.clear();
    CHECK(begin(pool, true, &h) == HOBBIT_EHIP); CHECK(raw::order.empty() && pool.parked() == (size_t)N);     // served from the pool, returned to it
}

int main() {
    test_buf(); CHECK(live() == 0);
    { test_grow(); } CHECK(live() == 0);
    test_pool(); CHECK(live() == 0);
    test_begin(); CHECK(live() == 0);
    puts("ok");
    return 0;
}
