// The lazy sums of csrc/hobbit_whir_acc.hpp against the eager form on the host's 128-bit path (tests/test_whir_long.py builds and runs this).
#include <cstdio>
#include <random>
#include "hobbit_whir_acc.hpp"
using namespace hobbit;
int main() {
    std::mt19937_64 g(12345);
    // canonical edge values: 0, 1, p - 1, both sides of the 31-bit limb boundary, all-ones low limb, all-ones high limb
    const uint64_t edge[] = {0, 1, 2, P61 - 1, P61 - 2, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1, 1ull << 30, 1ull << 60, (1ull << 60) - 1, P61 >> 1,
                             0x7FFFFFFFull << 30, 0x1FFFFFFF80000000ull, 0x1FFFFFFF7FFFFFFFull};
    const int ne = sizeof edge / sizeof edge[0];
    auto pick = [&](bool e) { return e ? edge[g() % ne] : g() % P61; };
    long bad = 0, tot = 0;
    for (int trial = 0; trial < 200000; trial++) {
        const int n = trial % 3 == 0 ? 1 + (int)(g() % 300) : 1 + (int)(g() % 16);
        const int mode = trial % 4;                      // 0: random, 1: both operands from the edge set, 2: a, 3: b
        LazyAcc s = lazy_zero(); F want = fmake(0);
        for (int i = 0; i < n; i++) {
            F a = fmake(pick(mode == 1 || mode == 2), pick(mode == 1 || mode == 2)), b = fmake(pick(mode == 1 || mode == 3), pick(mode == 1 || mode == 3));
            if (trial % 7 == 0) { a = fmake(P61 - 1, P61 - 1); b = fmake(P61 - 1, (i & 1) ? P61 - 1 : 0); }
            lazy_mad(s, a, b); want = fadd(want, fmul(a, b));
        }
        tot++;
        if (!feq(lazy_value(s), want)) { if (bad < 5) printf("mismatch: trial %d, %d products\n", trial, n); bad++; }
    }
    {   // the carry counts: 2^20 of the largest products in one sum
        const F a = fmake(P61 - 1, P61 - 1);
        LazyAcc s = lazy_zero(); F want = fmake(0);
        for (int i = 0; i < (1 << 20); i++) { lazy_mad(s, a, a); want = fadd(want, fmul(a, a)); }
        tot++;
        if (!feq(lazy_value(s), want)) { printf("mismatch: 2^20 largest products\n"); bad++; }
    }
    printf("%ld sums, %ld bad\n", tot, bad);
    return bad != 0;
}
