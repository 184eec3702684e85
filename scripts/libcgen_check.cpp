// libcgen_check.cpp -- stand-alone check of csrc/hobbit_libcgen.hpp (host arithmetic on glibc's TYPE_3 generator) against libc itself.
// No HIP, no library: build with the host compiler, with sanitizers if wanted, and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/libcgen_check.cpp -o /tmp/libcgen_check && /tmp/libcgen_check
// Exit status 0 and "libcgen_check ok" when every comparison holds.
#include <cstdio>
#include <vector>
#include "../hobbit-space-efficient-zksnark-with-optimal-prover-time_amd/csrc/hobbit_libcgen.hpp"

using namespace hobbit::libcgen;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::vector<uint32_t> libc_after(unsigned seed, uint64_t skip, int n) {
    srandom(seed);
    for (uint64_t i = 0; i < skip; i++) (void)random();
    std::vector<uint32_t> v(n);
    for (int i = 0; i < n; i++) v[i] = (uint32_t)(i & 1 ? rand() : random());
    return v;
}

int main() {
    uint32_t w[DEG], w2[DEG], w3[DEG];
    // snapshot + sequential model, and the snapshot disturbs nothing
    for (unsigned seed : {1u, 777u})
        for (uint64_t d : {0ull, 1ull, 30ull, 31ull, 32ull, 1000000ull}) {
            const std::vector<uint32_t> want = libc_after(seed, d, 100);
            srandom(seed); for (uint64_t i = 0; i < d; i++) (void)random();
            CHECK(snapshot(w) == 0, "snapshot seed %u d %llu", seed, (unsigned long long)d);
            for (int i = 0; i < 100; i++) { const uint32_t m = step(w), l = (uint32_t)random(); CHECK(m == want[i] && l == want[i], "seed %u d %llu draw %d: model %u libc %u want %u", seed, (unsigned long long)d, i, m, l, want[i]); }
        }
    // jump-ahead against sequential calls; write-back makes libc continue there
    for (uint64_t k : {0ull, 1ull, 2ull, 30ull, 31ull, 32ull, 100ull, (1ull << 20) + 7, 10000000ull}) {
        const std::vector<uint32_t> want = libc_after(5, k, 72);
        srandom(5); CHECK(snapshot(w) == 0, "snapshot");
        jump(w, k, w2);
        CHECK(write_back(w2) == 0, "write_back");
        for (int i = 0; i < 64; i++) { const uint32_t l = (uint32_t)rand(); CHECK(l == want[i], "jump %llu draw %d: libc %u want %u", (unsigned long long)k, i, l, want[i]); }
        // a second write-back while the library's own block is the active one (the next srandom then seeds that block)
        CHECK(snapshot(w3) == 0, "snapshot of the written-back state");
        CHECK(write_back(w3) == 0, "write_back onto the active block");
        for (int i = 64; i < 72; i++) { const uint32_t l = (uint32_t)random(); CHECK(l == want[i], "after the second write-back, draw %d: libc %u want %u", i, l, want[i]); }
    }
    // 64-bit k: composition only
    for (auto ab : {std::pair<uint64_t, uint64_t>{(1ull << 39) + 12345, (1ull << 39) - 999}, {(1ull << 62) + 77, (1ull << 62) - 5}}) {
        srandom(9); snapshot(w);
        jump(w, ab.first, w2); jump(w2, ab.second, w2);
        jump(w, ab.first + ab.second, w3);
        CHECK(!memcmp(w2, w3, sizeof w2), "jump(a) jump(b) != jump(a + b)");
    }
    // tables
    {
        std::vector<uint32_t> lt(DEG * 8), ct(DEG * 40);
        lane_table(124, 8, lt.data()); coarse_table(15872, 40, ct.data());
        srandom(3); snapshot(w);
        for (uint32_t l = 0; l < 8; l++) { Poly p; for (int j = 0; j < DEG; j++) p.c[j] = lt[j * 8 + l]; apply(p, w, w2); jump(w, 124ull * l, w3); CHECK(!memcmp(w2, w3, sizeof w2), "lane table %u", l); }
        for (int b : {0, 1, 17, 39}) { Poly p; memcpy(p.c, &ct[b * DEG], sizeof p.c); apply(p, w, w2); jump(w, 15872ull << b, w3); CHECK(!memcmp(w2, w3, sizeof w2), "coarse table %d", b); }
    }
    // a state that is not TYPE_3 is refused and left as it was
    for (size_t bytes : {(size_t)32, (size_t)64, (size_t)256}) {
        alignas(int32_t) static char a[256], b[256];
        initstate(11, a, bytes); const long x0 = random();
        initstate(11, b, bytes); CHECK(random() == x0, "control");
        std::vector<long> want(16); for (auto &v : want) v = random();
        initstate(11, a, bytes); (void)random();
        CHECK(snapshot(w) == -1, "snapshot of a %zu-byte state must fail", bytes);
        for (auto v : want) CHECK(random() == v, "%zu-byte state disturbed", bytes);
    }
    printf(fails ? "libcgen_check: %d failures\n" : "libcgen_check ok\n", fails);
    return fails != 0;
}
