// hobbit_whir_acc.hpp -- lazy sum of F_{p^2} products for the out-of-domain kernels of hobbit_whir.hip.
//
// hobbit_field.hpp's device product splits every component x = x0 + 2^31 x1 and forms, per output component, two sums of four 32 x 32
// products, L and M (each < 2^64), with  a b = L + 2^31 M (mod p)  folded once per product.  A sum of n products is  sum L + 2^31 sum M,  so
// the folds can wait: the four sums ride in 96 bits each (64 + a carry count), and one reduction at the end gives the canonical value.  Per
// product that is the sixteen multiply-adds and four three-instruction additions, against two folds and a canonical addition (some forty
// instructions) of  acc = fadd(acc, fmul(a, b)).  Exact integer arithmetic mod p throughout: the result has the bits of the eager form.
// Plain 32/64-bit C++, host and device: tests/whir_acc_check.cpp compares the host build with 128-bit arithmetic (tests/test_whir_long.py).
#pragma once
#include "hobbit_field.hpp"

namespace hobbit {

struct LazyAcc {
    uint64_t lr, mr, li, mi;          // low 64 bits of the four sums
    uint32_t hlr, hmr, hli, hmi;      // carries out of them: at most one per product, so n < 2^32 products
};
HB_HD LazyAcc lazy_zero() { LazyAcc s; s.lr = s.mr = s.li = s.mi = 0; s.hlr = s.hmr = s.hli = s.hmi = 0; return s; }
HB_HD uint64_t lazy_mad32(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }
HB_HD void lazy_add(uint64_t &lo, uint32_t &hi, uint64_t x) { const uint64_t s = lo + x; hi += s < x ? 1u : 0u; lo = s; }
// s += a * b; components of a and b <= p + 7 (canonical inputs are)
HB_HD void lazy_mad(LazyAcc &s, const F &a, const F &b) {
    const uint64_t nai = 2 * P61 - a.im;
    const uint32_t ar0 = (uint32_t)a.re & 0x7FFFFFFFu, ar1 = (uint32_t)(a.re >> 31), ai0 = (uint32_t)a.im & 0x7FFFFFFFu, ai1 = (uint32_t)(a.im >> 31);
    const uint32_t na0 = (uint32_t)nai & 0x7FFFFFFFu, na1 = (uint32_t)(nai >> 31);
    const uint32_t br0 = (uint32_t)b.re & 0x7FFFFFFFu, br1 = (uint32_t)(b.re >> 31), bi0 = (uint32_t)b.im & 0x7FFFFFFFu, bi1 = (uint32_t)(b.im >> 31);
    const uint32_t br1d = br1 << 1, bi1d = bi1 << 1;
    // each of the four is below 2^62 + 2^61 + 2^62 + 2^62 < 2^64 (hobbit_field.hpp, fmul_lazy)
    lazy_add(s.lr, s.hlr, lazy_mad32(na1, bi1d, lazy_mad32(na0, bi0, lazy_mad32(ar1, br1d, lazy_mad32(ar0, br0, 0)))));
    lazy_add(s.mr, s.hmr, lazy_mad32(na1, bi0, lazy_mad32(na0, bi1, lazy_mad32(ar1, br0, lazy_mad32(ar0, br1, 0)))));
    lazy_add(s.li, s.hli, lazy_mad32(ai1, br1d, lazy_mad32(ai0, br0, lazy_mad32(ar1, bi1d, lazy_mad32(ar0, bi0, 0)))));
    lazy_add(s.mi, s.hmi, lazy_mad32(ai1, br0, lazy_mad32(ai0, br1, lazy_mad32(ar1, bi0, lazy_mad32(ar0, bi1, 0)))));
}
// lo + 2^64 hi (mod p), canonical: 2^64 = 8, so the value is (lo mod 2^61) + (lo >> 61) + 8 hi < 2^61 + 8 + 2^35 < 2 p
HB_HD uint64_t lazy_fold96(uint64_t lo, uint32_t hi) {
    const uint64_t t = (lo & P61) + (lo >> 61) + ((uint64_t)hi << 3);
    return t >= P61 ? t - P61 : t;
}
// L + 2^31 M (mod p) for canonical L, M: 2^31 M = 2^31 (M mod 2^30) + (M >> 30) since 2^61 = 1; the sum is below 2^62 + 2^31
HB_HD uint64_t lazy_join(uint64_t L, uint64_t M) {
    uint64_t t = L + ((M & 0x3FFFFFFFull) << 31) + (M >> 30);
    t = (t & P61) + (t >> 61);
    return t >= P61 ? t - P61 : t;
}
HB_HD F lazy_value(const LazyAcc &s) {
    return fmake(lazy_join(lazy_fold96(s.lr, s.hlr), lazy_fold96(s.mr, s.hmr)), lazy_join(lazy_fold96(s.li, s.hli), lazy_fold96(s.mi, s.hmi)));
}

}  // namespace hobbit
