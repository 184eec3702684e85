// Stand-alone check of csrc/hobbit_fft_tables.hpp (the host-built twiddle tables of the FFT module), built by tests/test_fft_tables_cpu.py with
// g++, plain and with the address and undefined-behaviour sanitizers: the same builders the library uploads from.
// Every entry is compared with its definition, computed on its own by square-and-multiply from root_of_unity(logn); the inverse direction's
// w^-e is taken as rou^(N - e), so neither the power chain nor finv of the builders is used on the checking side.
// Prints "<check> <entries compared>" lines and exits 0, or names the first failure and exits 1.
#include <cstdio>
#include <vector>
#include "hobbit_fft_tables.hpp"

using namespace hobbit;

static int fail(const char *what, int logn, int inverse, unsigned long long at) { std::printf("FAIL %s logn=%d inverse=%d at=%llu\n", what, logn, inverse, at); return 1; }

// w^e for w = the order-2^logn root of unity (inverse: its inverse), any e
static F rootpow(int logn, bool inverse, unsigned long long e) {
    const unsigned long long N = 1ull << logn;
    e %= N;
    return fpow(root_of_unity(logn), inverse ? (N - e) % N : e);
}
static uint32_t bitrev3(uint32_t t) { return ((t & 1) << 2) | (t & 2) | ((t >> 2) & 1); }

static int check_roots(int logn, bool inv, unsigned long long &n) {
    const std::vector<F> t = fft::build_table(fft::ROOTS, logn, inv);
    if (t.size() != (logn >= 1 ? (size_t)1 << (logn - 1) : 1)) return fail("roots: size", logn, inv, t.size());
    for (size_t k = 0; k < t.size(); k++, n++) if (!feq(t[k], rootpow(logn, inv, k))) return fail("roots: entry", logn, inv, k);
    return 0;
}
static int check_radix8(int logn, bool inv, unsigned long long &n) {
    const std::vector<F> t = fft::build_table(fft::RADIX8, logn, inv);
    const uint32_t N = 1u << logn, P = (uint32_t)logn / 3, R = 1u << (logn % 3), N2 = N / R;
    size_t at = 0;
    uint32_t h = 8;
    for (uint32_t p = 1; p < P; p++, h *= 8)                    // pass tables [7][h]: w_N2^(rev3(t) k N2 / (8h)), w_N2 = w_N^R
        for (uint32_t b = 1; b < 8; b++)
            for (uint32_t k = 0; k < h; k++, at++, n++) {
                if (at >= t.size()) return fail("radix8: table too short", logn, inv, at);
                if (!feq(t[at], rootpow(logn, inv, (unsigned long long)R * bitrev3(b) * k * (N2 / (8 * h))))) return fail("radix8: pass entry", logn, inv, at);
            }
    for (uint32_t q = 1; q < R; q++)                            // tail [R-1][N2]: w_N^(q k)
        for (uint32_t k = 0; k < N2; k++, at++, n++) {
            if (at >= t.size()) return fail("radix8: table too short", logn, inv, at);
            if (!feq(t[at], rootpow(logn, inv, (unsigned long long)q * k))) return fail("radix8: tail entry", logn, inv, at);
        }
    if (at == 0) { if (t.size() != 1 || !feq(t[0], fmake(1))) return fail("radix8: the empty table must be the one entry 1", logn, inv, t.size()); n++; return 0; }
    if (at != t.size()) return fail("radix8: size", logn, inv, t.size());
    return 0;
}
static int check_split(int logn, bool inv, unsigned long long &n) {
    const std::vector<F> t = fft::build_table(fft::SPLIT, logn, inv);
    const size_t nlo = fft::SPLIT_LO, nhi = (size_t)1 << (logn - 14);
    if (nlo != ((size_t)1 << 14) || t.size() != nlo + nhi) return fail("split: size", logn, inv, t.size());
    const F *lo = t.data(), *hi = t.data() + nlo;
    auto ok = [&](size_t a, size_t b) { n++; return feq(fmul(hi[a], lo[b]), rootpow(logn, inv, ((unsigned long long)a << 14) + b)); };
    for (size_t a : {(size_t)0, (size_t)1, nhi - 1}) for (size_t b : {(size_t)0, (size_t)1, nlo - 1}) if (!ok(a, b)) return fail("split: corner", logn, inv, (a << 14) + b);
    uint64_t s = 0x9E3779B97F4A7C15ull;                        // fixed pseudo-random (a, b)
    for (int i = 0; i < 400; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull; const size_t a = (size_t)(s >> 33) % nhi;
        s = s * 6364136223846793005ull + 1442695040888963407ull; const size_t b = (size_t)(s >> 33) % nlo;
        if (!ok(a, b)) return fail("split: entry", logn, inv, (a << 14) + b);
    }
    return 0;
}

int main() {
    for (int inv = 0; inv < 2; inv++) {
        unsigned long long n = 0;
        for (int logn : {0, 1, 2, 7}) if (check_roots(logn, inv, n)) return 1;
        std::printf("roots_%s %llu\n", inv ? "inv" : "fwd", n);
        n = 0;
        for (int logn : {3, 5, 6, 7, 8, 11}) if (check_radix8(logn, inv, n)) return 1;
        std::printf("radix8_%s %llu\n", inv ? "inv" : "fwd", n);
        n = 0;
        if (check_radix8(12, inv, n)) return 1;                 // k_fft4096's [7][8] | [7][64] | [7][512]
        std::printf("radix8_4096_%s %llu\n", inv ? "inv" : "fwd", n);
        n = 0;
        if (check_split(25, inv, n)) return 1;
        std::printf("split_%s %llu\n", inv ? "inv" : "fwd", n);
        // the 8th roots the kernels take as arguments: powers of the order-4096 root; w4 = -i forward, +i inverse
        const fft::R8Roots c = fft::r8_roots(inv);
        if (!feq(c.w8, rootpow(12, inv, 512)) || !feq(c.w8_3, rootpow(12, inv, 1536)) || !feq(c.w4, rootpow(12, inv, 1024))) return fail("r8_roots", 12, inv, 0);
        if (!feq(c.w4, fmake(0, inv ? 1 : P61 - 1)) || !feq(fmul(c.w8, c.w8), c.w4) || !feq(fmul(c.w4, c.w8), c.w8_3)) return fail("r8_roots: w4 = -+i, w8^2 = w4", 12, inv, 0);
    }
    std::printf("r8_roots ok\n");
    return 0;
}
