// hobbit_libcgen.hpp -- host arithmetic on glibc's default generator (TYPE_3), the one rand() and random() share.  No HIP in here.
//
// The generator is the additive recurrence r_i = r_{i-3} + r_{i-31} mod 2^32; a draw returns r_i >> 1.  A WINDOW is the 31 words
// r_{i-31} .. r_{i-1} in sequence order (oldest first): draw 0 of a window is (w[28] + w[0]) >> 1.  The recurrence is linear over Z/2^32,
// so with p(x) = x^k mod (x^31 - x^28 - 1) = sum_j p_j x^j every word k places on is r_{m+k} = sum_j p_j r_{m+j}: the window k draws ahead
// costs O(log k) products of 31 x 31 words (pow_x) and one application (apply).
//
// State layout of glibc (stdlib/random_r.c): a block of 32 int32, word 0 = rear * 5 + type, then the ring of 31 words.  The next draw adds
// ring[rear] (r_{i-3}) into ring[(rear + 3) % 31] (r_{i-31}, the oldest) and returns that sum >> 1.  initstate() hands the caller's block
// back with word 0 brought up to date, setstate() of that pointer puts the caller's generator back undisturbed.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace hobbit { namespace libcgen {

constexpr int DEG = 31, SEP = 3, TYPE = 3, MAX_TYPES = 5;

struct Poly { uint32_t c[DEG]; };                       // sum_j c[j] x^j, reduced mod x^31 - x^28 - 1

inline Poly poly_const(uint32_t v) { Poly p; memset(p.c, 0, sizeof p.c); p.c[0] = v; return p; }
inline Poly poly_x() { Poly p; memset(p.c, 0, sizeof p.c); p.c[1] = 1; return p; }
inline Poly poly_mul(const Poly &a, const Poly &b) {
    uint32_t t[2 * DEG - 1] = {0};
    for (int i = 0; i < DEG; i++) for (int j = 0; j < DEG; j++) t[i + j] += a.c[i] * b.c[j];
    for (int d = 2 * DEG - 2; d >= DEG; d--) { t[d - SEP] += t[d]; t[d - DEG] += t[d]; }      // x^d = x^(d-3) + x^(d-31)
    Poly r; memcpy(r.c, t, sizeof r.c); return r;
}
// x^k mod (x^31 - x^28 - 1), any 64-bit k
inline Poly pow_x(uint64_t k) {
    Poly r = poly_const(1), b = poly_x();
    for (; k; k >>= 1) { if (k & 1) r = poly_mul(r, b); if (k >> 1) b = poly_mul(b, b); }
    return r;
}
// the 30 words that follow a window: ext[0..30] = w, ext[31 + t] = ext[28 + t] + ext[t]
inline void extend(const uint32_t w[DEG], uint32_t ext[2 * DEG - 1]) {
    memcpy(ext, w, DEG * sizeof(uint32_t));
    for (int t = 0; t < DEG - 1; t++) ext[DEG + t] = ext[DEG - SEP + t] + ext[t];
}
// out = the window that p = x^k carries w to: out[t] = sum_j p_j ext[t + j]   (out may alias w)
inline void apply(const Poly &p, const uint32_t w[DEG], uint32_t out[DEG]) {
    uint32_t ext[2 * DEG - 1]; extend(w, ext);
    for (int t = 0; t < DEG; t++) { uint32_t s = 0; for (int j = 0; j < DEG; j++) s += p.c[j] * ext[t + j]; out[t] = s; }
}
inline void jump(const uint32_t w[DEG], uint64_t k, uint32_t out[DEG]) { apply(pow_x(k), w, out); }
// one draw: the value libc would return, the window moved on by one
inline uint32_t step(uint32_t w[DEG]) {
    const uint32_t v = w[DEG - SEP] + w[0];
    memmove(w, w + 1, (DEG - 1) * sizeof(uint32_t)); w[DEG - 1] = v;
    return v >> 1;
}

// The caller's generator as a window.  0, or -1 when its state is not TYPE_3 (initstate with a buffer other than 128..255 bytes) or cannot be
// read; the generator is left exactly as it was either way.
inline int snapshot(uint32_t w[DEG]) {
    alignas(int32_t) char tmp[128];
    char *old = initstate(1u, tmp, sizeof tmp);
    if (!old) return -1;
    int32_t blk[DEG + 1]; memcpy(blk, old, sizeof blk);         // (word 0 was brought up to date by initstate)
    if (!setstate(old)) return -1;
    if (blk[0] < 0 || blk[0] % MAX_TYPES != TYPE) return -1;
    const int rear = blk[0] / MAX_TYPES;
    if (rear >= DEG) return -1;
    for (int j = 0; j < DEG; j++) w[j] = (uint32_t)blk[1 + (rear + SEP + j) % DEG];
    return 0;
}
// Make libc continue from window w.  The generator then runs on a block this function owns (process lifetime), as after an initstate of the
// caller's own; it is left through a temporary state first, so writing the block is safe when it is the active one.
inline int write_back(const uint32_t w[DEG]) {
    static int32_t blk[DEG + 1];
    alignas(int32_t) char tmp[128];
    if (!initstate(1u, tmp, sizeof tmp)) return -1;
    blk[0] = (DEG - SEP) * MAX_TYPES + TYPE;                    // rear = 28: the oldest word sits at ring index 0
    memcpy(blk + 1, w, DEG * sizeof(uint32_t));
    return setstate(reinterpret_cast<char *>(blk)) ? 0 : -1;
}
// The reference's transcript is a function of the process-wide libc generator (rand()/random(), never seeded: SURVEY.md 0.8).
// Initialising the HIP runtime draws from that same generator (measured: srandom(1); <first HIP call>; rand() no longer returns
// 1804289383), so everything that can trigger runtime initialisation -- device query, stream creation, the first allocation, the
// first kernel launch of a file (code-object load) -- runs with the generator parked on a private state for the lifetime of a Guard,
// and the caller's state is put back untouched.
struct Guard {
    alignas(int32_t) char tmp[256]; char *prev;
    Guard() { prev = initstate(0x9e3779b9u, tmp, sizeof tmp); }
    ~Guard() { if (prev) setstate(prev); }
    Guard(const Guard &) = delete; Guard &operator=(const Guard &) = delete;
};

// Jump tables of the kernels (hobbit_libcgen.hip).
// lane table, transposed for coalesced reads: out[j * lanes + l] = coefficient j of x^(l * run)
inline void lane_table(uint32_t run, uint32_t lanes, uint32_t *out) {
    const Poly s = pow_x(run); Poly p = poly_const(1);
    for (uint32_t l = 0; l < lanes; l++) { for (int j = 0; j < DEG; j++) out[(size_t)j * lanes + l] = p.c[j]; p = poly_mul(p, s); }
}
// coarse table: out[b * 31 + j] = coefficient j of x^(stride * 2^b), b < nbits
inline void coarse_table(uint64_t stride, int nbits, uint32_t *out) {
    Poly p = pow_x(stride);
    for (int b = 0; b < nbits; b++) { memcpy(out + (size_t)b * DEG, p.c, sizeof p.c); p = poly_mul(p, p); }
}

}}  // namespace hobbit::libcgen
