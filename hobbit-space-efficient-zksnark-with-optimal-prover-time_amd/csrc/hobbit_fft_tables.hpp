// hobbit_fft_tables.hpp -- the host-built twiddle tables of the FFT module (hobbit_fft.hip), as pure functions of (kind, logn, direction).
// No HIP: tests/fft_tables_check.cpp builds them with g++ and checks every entry against the definition.
#pragma once
#include <vector>
#include "hobbit_field.hpp"

namespace hobbit { namespace fft {

enum Kind {
    ROOTS,      // w^k, k < 2^(logn-1) (one entry for logn = 0): w[1] = rou or its inverse, w[i] = w[i-1] w[1] (src/utils.cpp:646-653)
    RADIX8,     // the radix-8 kernels, N = 2^logn = 8^P R: per pass p = 1 .. P-1 with octet stride h = 8^p, for t = 1..7 and k < h,
                // T[t-1][k] = w_N2^(rev3(t) k N2 / (8h)), w_N2 = w_N^R, N2 = N / R (block t of an octet holds the sub-transform of the samples
                // = rev3(t) mod 8); then the tail [R-1][N2] = w_N^(q k); one entry (1) where there is neither.  logn = 12: k_fft4096's
                // [7][8] | [7][64] | [7][512]
    SPLIT,      // lengths 2^25 .. 2^28 as two small tables, w^(a 2^14 + b) = hi[a] lo[b]: [lo: 2^14 | hi: 2^(logn-14)] entries, at most 512 KB together,
                // each built by its own short chain of products (the full table would be 2^27 dependent products and a 2 GiB upload)
    TW2D        // [n1][k2] = w^(n1 k2), 2^logn entries (up to 32 MB): built on the device (k_build_tw2d), never here
};
constexpr size_t SPLIT_LO = (size_t)1 << 14;

inline F root(int logn, bool inverse) { const F w = root_of_unity(logn); return inverse ? finv(w) : w; }
// 1, w, w^2, ... (n entries), each the product of the one before with w
inline std::vector<F> power_chain(const F &w, size_t n) {
    std::vector<F> t(n);
    t[0] = fmake(1);
    for (size_t i = 1; i < n; i++) t[i] = fmul(t[i - 1], w);
    return t;
}
inline std::vector<F> build_table(Kind kind, int logn, bool inverse) {
    const F w1 = root(logn, inverse);
    if (kind == ROOTS) return power_chain(w1, logn >= 1 ? (size_t)1 << (logn - 1) : 1);
    if (kind == SPLIT) {
        std::vector<F> t = power_chain(w1, SPLIT_LO);
        const std::vector<F> hi = power_chain(fmul(t[SPLIT_LO - 1], w1), (size_t)1 << (logn - 14));      // w^(2^14)
        t.insert(t.end(), hi.begin(), hi.end());
        return t;
    }
    const uint32_t N = 1u << logn, P = (uint32_t)logn / 3, R = 1u << (logn % 3), N2 = N / R;
    const std::vector<F> w = power_chain(w1, N);
    static const uint32_t rev3[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    std::vector<F> t;
    uint32_t h = 8;
    for (uint32_t p = 1; p < P; p++, h *= 8)
        for (uint32_t b = 1; b < 8; b++) for (uint32_t k = 0; k < h; k++) t.push_back(w[(size_t)R * ((rev3[b] * k * (N2 / (8 * h))) % N2)]);
    for (uint32_t q = 1; q < R; q++) for (uint32_t k = 0; k < N2; k++) t.push_back(w[((size_t)q * k) % N]);
    if (t.empty()) t.push_back(fmake(1));
    return t;
}
// the 8th roots that k_fft4096 and the radix-8 kernels take as arguments: w8, w8^3 and w4 = +-i of the direction (the same for every length)
struct R8Roots { F w8, w8_3, w4; };
inline R8Roots r8_roots(bool inverse) { const F w = root(12, inverse); return {fpow(w, 512), fpow(w, 1536), fpow(w, 1024)}; }

}}  // namespace hobbit::fft
