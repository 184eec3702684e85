/* oracle/hobbit_oracle.c -- TEST INFRASTRUCTURE ONLY (see hobbit_oracle.h).
 *
 * A plain-C, single-threaded restatement of the reference's Our_PC / Elastic_PC commit path and
 * in-memory sumchecks.  It is written from the reference's *behaviour* (each function cites the
 * reference file:line it follows); it shares no code with it.  It is the checker for the HIP
 * path, never the thing shipped or measured (bench.py times it only as "cpu_baseline", kind
 * "port").  Parity status: PINNED against oracle/_ref (the real reference) -- see header.
 *
 * All arithmetic is exact integer arithmetic in F_{p^2}, p = 2^61-1, i^2 = -1, with canonical
 * outputs 0 <= re,im < p (reference: src/fieldElement.cpp:34-96,336-360 produces canonical
 * outputs for canonical inputs, so any algebraically equal evaluation order is bit-identical).
 */
#define _GNU_SOURCE
#include "hobbit_oracle.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef unsigned __int128 u128;
#define P61 2305843009213693951ULL

/* ------------------------------------------------------------------------------------------ */
/* field: src/fieldElement.cpp:34-47 (+), 80-96 (-), 49-78 (*), 206-209 (inv), 237-249 (rou)    */
/* ------------------------------------------------------------------------------------------ */
static inline uint64_t red128(u128 x) { /* x < 2^125 */
    u128 s = (x & P61) + (x >> 61);
    uint64_t t = (uint64_t)(s & P61) + (uint64_t)(s >> 61);
    return t >= P61 ? t - P61 : t;
}
static inline uint64_t addp(uint64_t a, uint64_t b) { uint64_t s = a + b; return s >= P61 ? s - P61 : s; }
static inline uint64_t subp(uint64_t a, uint64_t b) { return a >= b ? a - b : a + P61 - b; }
static inline oF f_add(oF a, oF b) { oF r = {addp(a.re, b.re), addp(a.im, b.im)}; return r; }
static inline oF f_sub(oF a, oF b) { oF r = {subp(a.re, b.re), subp(a.im, b.im)}; return r; }
static inline oF f_mul(oF a, oF b) {
    uint64_t ac = red128((u128)a.re * b.re), bd = red128((u128)a.im * b.im);
    uint64_t all = red128((u128)(a.re + a.im) * (b.re + b.im));
    oF r = {subp(ac, bd), subp(subp(all, ac), bd)};
    return r;
}
static inline oF fint(uint64_t x) { oF r = {x, 0}; return r; }
static inline int fis0(oF a) { return a.re == 0 && a.im == 0; }
static oF finv(oF x) { /* x^(p^2-2), square-and-multiply LSB first as fastPow (fieldElement.cpp:318-333) */
    u128 e = (u128)P61 * P61 - 2;
    oF ret = fint(1), tmp = x;
    while (e) { if (e & 1) ret = f_mul(ret, tmp); tmp = f_mul(tmp, tmp); e >>= 1; }
    return ret;
}
static oF root_of_unity(int logn) { /* src/utils.cpp:452-463 */
    oF r = {2147483648ULL, 1033321771269002680ULL};
    for (int i = 0; i < 62 - logn; i++) r = f_mul(r, r);
    return r;
}
void orc_f_add(const oF *a, const oF *b, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = f_add(a[i], b[i]); }
void orc_f_sub(const oF *a, const oF *b, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = f_sub(a[i], b[i]); }
void orc_f_mul(const oF *a, const oF *b, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = f_mul(a[i], b[i]); }
void orc_f_neg(const oF *a, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = f_sub(fint(0), a[i]); }
void orc_f_inv(const oF *a, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = finv(a[i]); }
void orc_root_of_unity(int logn, oF *o) { *o = root_of_unity(logn); }

/* ------------------------------------------------------------------------------------------ */
/* mimc: src/mimc.cpp:4 (161 rounds), 11-19 (constants F(i)), 95-107                            */
/* ------------------------------------------------------------------------------------------ */
static oF mimc_hash(oF x, oF k) {
    oF h = fint(0), t;
    for (int i = 0; i < 161; i++) {
        t = i == 0 ? f_add(x, k) : f_add(f_add(h, k), fint((uint64_t)(i - 1)));
        h = f_mul(f_mul(t, t), t);
    }
    return f_add(h, k);
}
void orc_mimc(const oF *x, const oF *k, oF *o, size_t n) { for (size_t i = 0; i < n; i++) o[i] = mimc_hash(x[i], k[i]); }

/* ------------------------------------------------------------------------------------------ */
/* BLAKE3 of exactly 64 bytes: src/Blake3_hash.cpp:5-10 = one compression with the IV as key,   */
/* counter 0, block_len 64, flags CHUNK_START|CHUNK_END|ROOT (Blake/blake3.c:146-151,598-617;   */
/* round function Blake/blake3_portable.c).  Restated from the BLAKE3 specification.            */
/* ------------------------------------------------------------------------------------------ */
static const uint32_t B3_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
static const uint8_t B3_PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
static inline uint32_t rotr32(uint32_t x, int c) { return (x >> c) | (x << (32 - c)); }
#define B3G(a, b, c, d, x, y) do { \
    v[a] = v[a] + v[b] + (x); v[d] = rotr32(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr32(v[b] ^ v[c], 12); \
    v[a] = v[a] + v[b] + (y); v[d] = rotr32(v[d] ^ v[a], 8);  v[c] = v[c] + v[d]; v[b] = rotr32(v[b] ^ v[c], 7); } while (0)
static void blake3_64(const uint8_t in[64], uint8_t out[32]) {
    uint32_t m[16], v[16], t[16];
    memcpy(m, in, 64); /* little-endian host */
    for (int i = 0; i < 8; i++) v[i] = B3_IV[i];
    v[8] = B3_IV[0]; v[9] = B3_IV[1]; v[10] = B3_IV[2]; v[11] = B3_IV[3];
    v[12] = 0; v[13] = 0; v[14] = 64; v[15] = 1 | 2 | 8;
    for (int r = 0; r < 7; r++) {
        B3G(0, 4, 8, 12, m[0], m[1]);   B3G(1, 5, 9, 13, m[2], m[3]);
        B3G(2, 6, 10, 14, m[4], m[5]);  B3G(3, 7, 11, 15, m[6], m[7]);
        B3G(0, 5, 10, 15, m[8], m[9]);  B3G(1, 6, 11, 12, m[10], m[11]);
        B3G(2, 7, 8, 13, m[12], m[13]); B3G(3, 4, 9, 14, m[14], m[15]);
        for (int i = 0; i < 16; i++) t[i] = m[B3_PERM[i]];
        memcpy(m, t, 64);
    }
    for (int i = 0; i < 8; i++) v[i] ^= v[i + 8];
    memcpy(out, v, 32);
}
void orc_blake3_64(const uint8_t *in, uint8_t *out, size_t n) { for (size_t i = 0; i < n; i++) blake3_64(in + 64 * i, out + 32 * i); }

/* src/merkle_tree.cpp:62-87: H( H(x|y|z|w) | prev ) */
static void hash_md(const oF xyzw[4], const uint8_t prev[32], uint8_t out[32]) {
    uint8_t d[64];
    memcpy(d, xyzw, 64);
    blake3_64(d, d);           /* inner digest into d[0..32) (blake3_64 copies its input first) */
    memcpy(d + 32, prev, 32);
    blake3_64(d, out);
}
void orc_hash_md(const oF *xyzw, const uint8_t *prev, uint8_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) { uint8_t p[32]; memcpy(p, prev + 32 * i, 32); hash_md(xyzw + 4 * i, p, out + 32 * i); }
}
/* src/merkle_tree.cpp:255-287: parent = H(left | left) -- the right child is never read. */
static size_t create_tree(uint8_t *levels, size_t n) {
    size_t off = 0, tot = n;
    uint8_t d[64];
    for (size_t sz = n / 2; sz >= 1; sz /= 2) {
        uint8_t *prev = levels + 32 * off, *cur = levels + 32 * tot;
        for (size_t i = 0; i < sz; i++) { memcpy(d, prev + 64 * i, 32); memcpy(d + 32, prev + 64 * i, 32); blake3_64(d, cur + 32 * i); }
        off = tot; tot += sz;
    }
    return tot;
}
size_t orc_create_tree_blake(const uint8_t *level0, size_t n, uint8_t *levels_out) {
    memmove(levels_out, level0, 32 * n);
    return create_tree(levels_out, n);
}
/* src/merkle_tree.cpp:193-221: leaf i = H(4 consecutive F), then the tree */
size_t orc_mt_commit_blake(const oF *leafs, size_t N, uint8_t *levels_out) {
    for (size_t i = 0; i < N / 4; i++) blake3_64((const uint8_t *)(leafs + 4 * i), levels_out + 32 * i);
    return create_tree(levels_out, N / 4);
}
/* src/merkle_tree.cpp:308-324 */
int orc_open_tree_blake(const uint8_t *levels, size_t n_leaves, size_t col, size_t row, size_t columns, uint8_t *path_out) {
    size_t pos = (row / 4) * columns + col, off = 0;
    int depth = 0;
    if (pos >= n_leaves) return -1;
    for (size_t sz = n_leaves; sz > 1; sz /= 2) {
        size_t sib = 2 * (pos / 2) + (1 - (pos % 2));
        memcpy(path_out + 32 * depth, levels + 32 * (off + sib), 32);
        pos /= 2; off += sz; depth++;
    }
    return depth;
}

/* ------------------------------------------------------------------------------------------ */
/* libc RNG.  glibc's rand() and random() are one generator (default seed 1); the reference     */
/* never seeds it on the live path, so srandom(1) == fresh-process state.          */
/* ------------------------------------------------------------------------------------------ */
void orc_rng_reset(void) { srandom(1); }
/* src/utils.cpp:873-883 */
void orc_generate_randomness(int n, oF *out) {
    oF c = fint(0);
    for (int i = 0; i < n; i++) {
        if (i % 100 == 0) c = fint((uint64_t)random());
        out[i] = f_add(c, fint((uint64_t)rand()));
    }
}

/* ------------------------------------------------------------------------------------------ */
/* expander graphs: src/expanders.h:20-47 (draw), 78-92 (recursion); src/parameter.h:4-8        */
/* ------------------------------------------------------------------------------------------ */
#define ORC_MAXDEP 100
typedef struct { long long L, R; int degree; long long *nbr; oF *w; } ograph;
static ograph gC[ORC_MAXDEP], gD[ORC_MAXDEP];
static const double k_alpha = 0.211, k_r = 1.72;
static const int k_cn = 9, k_dn = 12;
static const int k_dist_thr = (int)(1.0 / 0.07) - 1; /* 13 */

static void graph_draw(ograph *g, long long L, long long R, int d) {
    free(g->nbr); free(g->w);
    g->L = L; g->R = R; g->degree = d;
    g->nbr = (long long *)malloc(sizeof(long long) * (size_t)(L * d + 1));
    g->w = (oF *)malloc(sizeof(oF) * (size_t)(L * d + 1));
    for (long long i = 0; i < L; i++)
        for (int j = 0; j < d; j++) {
            long long target = rand() % R;          /* expanders.h:36 */
            long long weight = random();            /* expanders.h:37 */
            g->nbr[i * d + j] = target;
            g->w[i * d + j] = fint((uint64_t)weight);
        }
}
static long long expander_init(long long n, int dep) {
    if (n <= k_dist_thr) return n;
    graph_draw(&gC[dep], n, (long long)(k_alpha * n), k_cn);
    long long L = expander_init((long long)(k_alpha * n), dep + 1);
    graph_draw(&gD[dep], L, (long long)(n * (k_r - 1) - L), k_dn);
    return n + L + (long long)(n * (k_r - 1) - L);
}
long long orc_expander_init_store(long long n) { return expander_init(n, 0); }
long long orc_graph_dims(int dep, int kind, long long *R, int *degree) {
    ograph *g = kind ? &gD[dep] : &gC[dep]; *R = g->R; *degree = g->degree; return g->L;
}
void orc_graph_edges(int dep, int kind, long long *nbr, oF *w) {
    ograph *g = kind ? &gD[dep] : &gC[dep];
    memcpy(nbr, g->nbr, sizeof(long long) * (size_t)(g->L * g->degree));
    memcpy(w, g->w, sizeof(oF) * (size_t)(g->L * g->degree));
}
void orc_graph_set_weights(int dep, int kind, const oF *w) {
    ograph *g = kind ? &gD[dep] : &gC[dep];
    memcpy(g->w, w, sizeof(oF) * (size_t)(g->L * g->degree));
}
/* any graph of the drawn shape: L, R and degree stay, neighbours (each in [0, R)) and weights are replaced; -1 and nothing changed if a
 * neighbour is out of range */
int orc_graph_set_edges(int dep, int kind, const long long *nbr, const oF *w) {
    ograph *g = kind ? &gD[dep] : &gC[dep];
    size_t m = (size_t)(g->L * g->degree);
    for (size_t e = 0; e < m; e++) if (nbr[e] < 0 || nbr[e] >= g->R) return -1;
    memcpy(g->nbr, nbr, sizeof(long long) * m);
    memcpy(g->w, w, sizeof(oF) * m);
    return 0;
}

/* src/linear_code_encode.h:62-119: codeword = [x | Enc(C x) | D Enc(C x)] by scatter-add */
static long long encode_rec(const oF *src, oF *dst, long long n, int dep) {
    if (n <= k_dist_thr) { for (long long i = 0; i < n; i++) dst[i] = src[i]; return n; }
    const ograph *C = &gC[dep], *D = &gD[dep];
    long long R = (long long)(k_alpha * n);
    oF *s1 = (oF *)calloc((size_t)R + 1, sizeof(oF));
    for (long long i = 0; i < n; i++) dst[i] = src[i];
    for (long long i = 0; i < n; i++)
        for (int d = 0; d < C->degree; d++) {
            long long t = C->nbr[i * C->degree + d];
            s1[t] = f_add(s1[t], f_mul(C->w[i * C->degree + d], src[i]));
        }
    long long L = encode_rec(s1, dst + n, R, dep + 1);
    free(s1);
    R = D->R;
    for (long long i = 0; i < R; i++) dst[n + L + i] = fint(0);
    for (long long i = 0; i < L; i++)
        for (int d = 0; d < D->degree; d++) {
            long long t = D->nbr[i * D->degree + d];
            dst[n + L + t] = f_add(dst[n + L + t], f_mul(dst[n + i], D->w[i * D->degree + d]));
        }
    return n + L + R;
}
/* dst holds 2n F; the tail past the codeword stays 0 as in the callers' vector<F>(2n, F(0)) */
int orc_encode_monolithic(const oF *src, oF *dst, long long n) {
    memset(dst, 0, sizeof(oF) * (size_t)(2 * n));
    oF *tmp = (oF *)calloc((size_t)(2 * n) + 16, sizeof(oF));
    long long len = encode_rec(src, tmp, n, 0);
    memcpy(dst, tmp, sizeof(oF) * (size_t)len);
    free(tmp);
    return (int)len;
}

/* ------------------------------------------------------------------------------------------ */
/* FFT: src/utils.cpp:467-527 (fft, fresh twiddles) and 605-673 (_fft, twiddle cache `w` keyed   */
/* on the length only -- an inverse call at a cached length reuses forward twiddles: quirk kept) */
/* ------------------------------------------------------------------------------------------ */
static oF *g_w = NULL; static uint32_t g_wlen = 0;
void orc_fft_cache_reset(void) { free(g_w); g_w = NULL; g_wlen = 0; }
static void fft_core(oF *arr, int logn, int inverse, const oF *w) {
    uint32_t len = 1u << logn;
    uint32_t *rev = (uint32_t *)malloc(sizeof(uint32_t) * len);
    rev[0] = 0;
    for (uint32_t i = 1; i < len; i++) rev[i] = (rev[i >> 1] >> 1) | ((i & 1) << (logn - 1));
    for (uint32_t i = 0; i < len; i++) if (rev[i] < i) { oF t = arr[i]; arr[i] = arr[rev[i]]; arr[rev[i]] = t; }
    free(rev);
    for (uint32_t i = 2; i <= len; i <<= 1)
        for (uint32_t j = 0; j < len; j += i)
            for (uint32_t k = 0; k < (i >> 1); k++) {
                oF u = arr[j + k], v = f_mul(arr[j + k + (i >> 1)], w[len / i * k]);
                arr[j + k] = f_add(u, v);
                arr[j + k + (i >> 1)] = f_sub(u, v);
            }
    if (inverse) {
        oF ilen = finv(fint(len));
        for (uint32_t i = 0; i < len; i++) arr[i] = f_mul(arr[i], ilen);
    }
}
static void make_twiddles(oF *w, int logn, int inverse) {
    uint32_t len = 1u << logn;
    w[0] = fint(1);
    if (len > 1) { w[1] = root_of_unity(logn); if (inverse) w[1] = finv(w[1]); }
    for (uint32_t i = 2; i < len; i++) w[i] = f_mul(w[i - 1], w[1]);
}
void orc_fft(oF *arr, int logn, int inverse) {
    uint32_t len = 1u << logn;
    oF *w = (oF *)malloc(sizeof(oF) * (len + 2));
    make_twiddles(w, logn, inverse);
    fft_core(arr, logn, inverse, w);
    free(w);
}
void orc_fft_cached(oF *arr, int logn, int inverse) {
    uint32_t len = 1u << logn;
    if (g_wlen != len) { free(g_w); g_w = (oF *)malloc(sizeof(oF) * (len + 2)); g_wlen = len; make_twiddles(g_w, logn, inverse); }
    fft_core(arr, logn, inverse, g_w);
}

/* src/utils.cpp:251-296 */
void orc_precompute_beta(const oF *r, int k, oF *out) {
    size_t n = (size_t)1 << k;
    oF *tmp = (oF *)malloc(sizeof(oF) * n);
    out[0] = fint(1);
    for (int i = 0; i < k; i++) {
        size_t m = (size_t)1 << i;
        memcpy(tmp, out, sizeof(oF) * m);
        for (size_t j = 0; j < m; j++) {
            oF t = f_mul(r[k - 1 - i], tmp[j]);
            out[2 * j] = f_sub(tmp[j], t);
            out[2 * j + 1] = t;
        }
    }
    free(tmp);
}
/* src/utils.cpp:789-802 */
void orc_evaluate_vector(const oF *v_in, size_t n, const oF *r, int k, oF *out) {
    int lg = (int)log2((double)n);
    (void)k;
    oF *v = (oF *)malloc(sizeof(oF) * n);
    memcpy(v, v_in, sizeof(oF) * n);
    for (int i = 0; i < lg; i++) {
        size_t L = (size_t)1 << (lg - 1 - i);
        for (size_t j = 0; j < L; j++) v[j] = f_add(f_mul(f_sub(fint(1), r[i]), v[2 * j]), f_mul(r[i], v[2 * j + 1]));
    }
    *out = v[0];
    free(v);
}

/* ------------------------------------------------------------------------------------------ */
/* tensor code: src/PC_utils.cpp:66-123.  out is row-major (2*trs) x (2*M/trs).                 */
/* ------------------------------------------------------------------------------------------ */
void orc_compute_tensorcode(const oF *msg, size_t M, int trs, int lin, oF *out) {
    size_t cols = 2 * M / (size_t)trs, half = M / (size_t)trs, rows = 2 * (size_t)trs;
    memset(out, 0, sizeof(oF) * rows * cols);
    for (size_t i = 0; i < (size_t)trs; i++) memcpy(out + i * cols, msg + i * half, sizeof(oF) * half);
    int logc = (int)log2((double)cols);
    for (size_t i = 0; i < (size_t)trs; i++) orc_fft_cached(out + i * cols, logc, 0);
    oF *buf = (oF *)malloc(sizeof(oF) * rows), *buf2 = (oF *)malloc(sizeof(oF) * rows);
    for (size_t c = 0; c < cols; c++) {
        if (!lin) {
            for (size_t j = 0; j < rows; j++) buf[j] = j < (size_t)trs ? out[j * cols + c] : fint(0);
            orc_fft_cached(buf, (int)log2((double)rows), 0);
            for (size_t j = 0; j < rows; j++) out[j * cols + c] = buf[j];
        } else {
            for (size_t j = 0; j < (size_t)trs; j++) buf[j] = out[j * cols + c];
            orc_encode_monolithic(buf, buf2, trs);
            for (size_t j = 0; j < rows; j++) out[j * cols + c] = buf2[j];
        }
    }
    free(buf); free(buf2);
}

/* src/Our_PC.cpp:146-171.  levels_out: (2M-1)*32 bytes; tensor_out: NULL or K*(2trs)*(2M/trs) F */
size_t orc_commit_standard(const oF *poly, size_t N, int K, int trs, int lin, uint8_t *levels_out, oF *tensor_out) {
    size_t M = N / (size_t)K, cols = 2 * M / (size_t)trs, rows = 2 * (size_t)trs;
    oF *t = (oF *)malloc(sizeof(oF) * rows * cols);
    memset(levels_out, 0, 32 * M);
    for (int i = 0; i < K; i++) {
        orc_compute_tensorcode(poly + (size_t)i * M, M, trs, lin, t);
        if (tensor_out) memcpy(tensor_out + (size_t)i * rows * cols, t, sizeof(oF) * rows * cols);
        for (size_t j = 0; j < (size_t)trs / 2; j++)
            for (size_t k = 0; k < cols; k++) {
                oF x[4] = {t[(4 * j) * cols + k], t[(4 * j + 1) * cols + k], t[(4 * j + 2) * cols + k], t[(4 * j + 3) * cols + k]};
                uint8_t *leaf = levels_out + 32 * (j * cols + k);
                hash_md(x, leaf, leaf);
            }
    }
    free(t);
    return create_tree(levels_out, M);
}
/* src/Our_PC.cpp:258-272 (axpy part of _aggregate) */
void orc_aggregate(const oF *poly, size_t N, const oF *beta, int K, oF *aggr_out) {
    size_t M = N / (size_t)K;
    for (size_t j = 0; j < M; j++) aggr_out[j] = fint(0);
    for (int i = 0; i < K; i++)
        for (size_t j = 0; j < M; j++) aggr_out[j] = f_add(aggr_out[j], f_mul(beta[i], poly[(size_t)i * M + j]));
}

/* ------------------------------------------------------------------------------------------ */
/* sumchecks.  Round polynomials are coefficient triples/quadruples, highest degree first       */
/* (src/polynomial.h:18-70; products src/polynomial.cpp:91-147).                                */
/* ------------------------------------------------------------------------------------------ */
/* src/sumcheck.cpp:2391-2460: hash the round polynomial FIRST, then fold with the new challenge */
void orc_sumcheck2(const oF *_v1, const oF *_v2, size_t n, const oF *prev_r, oF *qpoly, oF *r, oF *vr, oF *fin) {
    int rounds = (int)log2((double)n);
    oF *v1 = (oF *)malloc(sizeof(oF) * (n / 2 + 1)), *v2 = (oF *)malloc(sizeof(oF) * (n / 2 + 1));
    oF rnd = *prev_r;
    for (int i = 0; i < rounds; i++) {
        const oF *a = i == 0 ? _v1 : v1, *b = i == 0 ? _v2 : v2;
        size_t L = (size_t)1 << (rounds - 1 - i);
        oF pa = fint(0), pb = fint(0), pc = fint(0);
        for (size_t j = 0; j < L; j++) {
            oF l1a = f_sub(a[2 * j + 1], a[2 * j]), l1b = a[2 * j];
            oF l2a = f_sub(b[2 * j + 1], b[2 * j]), l2b = b[2 * j];
            pa = f_add(pa, f_mul(l1a, l2a));
            pb = f_add(pb, f_add(f_mul(l1a, l2b), f_mul(l1b, l2a)));
            pc = f_add(pc, f_mul(l1b, l2b));
        }
        rnd = mimc_hash(rnd, pa); rnd = mimc_hash(rnd, pb); rnd = mimc_hash(rnd, pc);
        r[i] = rnd; qpoly[3 * i] = pa; qpoly[3 * i + 1] = pb; qpoly[3 * i + 2] = pc;
        for (size_t j = 0; j < L; j++) {
            oF x = f_add(a[2 * j], f_mul(rnd, f_sub(a[2 * j + 1], a[2 * j])));
            oF y = f_add(b[2 * j], f_mul(rnd, f_sub(b[2 * j + 1], b[2 * j])));
            v1[j] = x; v2[j] = y;
        }
    }
    rnd = mimc_hash(rnd, v1[0]); rnd = mimc_hash(rnd, v2[0]);
    vr[0] = v1[0]; vr[1] = v2[0]; *fin = rnd;
    free(v1); free(v2);
}
/* Degree-4 gate-consistency sumcheck, src/sumcheck.cpp:875-929 (the in-memory phase of prove_gate_consistency after the
 * streaming folds): sum over the six folded tables of  add*beta*(a0 L + a1 R) + a2*mul*beta*L*R + a3*beta*O.
 * Tables (n each, folded IN PLACE, adjacent pairs 2j,2j+1): t[0]=fold_add, t[1]=fold_beta, t[2]=fold_L, t[3]=fold_R, t[4]=fold_O,
 * t[5]=fold_mul.  Note the transcript order mimc_hash(coefficient, rand) (coefficient is the INPUT, rand the key).
 * poly: rounds x 5 (a..e, highest degree first); r: rounds; fin: the six t[i][0]; *check = every "Error in gate consistency 2"
 * comparison held; *sum_io: claimed sum in, last poly.eval(rand) out; *rand_io: transcript state in/out.
 * NOT pinned against oracle/_ref as a whole: the loop is inline in prove_gate_consistency, which only runs on the witness
 * stream machinery (out of scope); the linear_poly products follow src/polynomial.cpp:91-147, which sumcheck2/3 pin. */
void orc_gate_claim(oF *const t[6], size_t n, const oF *a, oF *out) {
    oF s = fint(0);
    for (size_t j = 0; j < n; j++) {
        oF lr = f_add(f_mul(a[0], t[2][j]), f_mul(a[1], t[3][j]));
        oF x = f_mul(f_mul(t[0][j], t[1][j]), lr);
        oF y = f_mul(a[2], f_mul(f_mul(t[5][j], t[1][j]), f_mul(t[2][j], t[3][j])));
        oF z = f_mul(a[3], f_mul(t[1][j], t[4][j]));
        s = f_add(s, f_add(x, f_add(y, z)));
    }
    *out = s;
}
void orc_gate_sumcheck(oF *t0, oF *t1, oF *t2, oF *t3, oF *t4, oF *t5, size_t n, const oF *a, oF *rand_io, oF *sum_io, oF *poly, oF *r, oF *fin, int *check) {
    oF *t[6] = {t0, t1, t2, t3, t4, t5};
    int rounds = (int)log2((double)n);
    oF rnd = *rand_io, sum = *sum_io;
    *check = 1;
    for (int rd = 0, i = rounds - 1; i >= 0; i--, rd++) {
        size_t L = (size_t)1 << i;
        oF c1[4] = {fint(0), fint(0), fint(0), fint(0)}, c4[5] = {fint(0), fint(0), fint(0), fint(0), fint(0)}, c2[3] = {fint(0), fint(0), fint(0)};
        for (size_t j = 0; j < L; j++) {
            oF d[6], b[6];
            for (int q = 0; q < 6; q++) { b[q] = t[q][2 * j]; d[q] = f_sub(t[q][2 * j + 1], b[q]); }
            /* l1 = add, l2 = beta, l3 = a0 L + a1 R  -> cubic */
            oF l3a = f_add(f_mul(a[0], d[2]), f_mul(a[1], d[3])), l3b = f_add(f_mul(a[0], b[2]), f_mul(a[1], b[3]));
            oF qa = f_mul(d[0], d[1]), qb = f_add(f_mul(d[0], b[1]), f_mul(b[0], d[1])), qc = f_mul(b[0], b[1]);
            c1[0] = f_add(c1[0], f_mul(qa, l3a));
            c1[1] = f_add(c1[1], f_add(f_mul(qa, l3b), f_mul(qb, l3a)));
            c1[2] = f_add(c1[2], f_add(f_mul(qb, l3b), f_mul(qc, l3a)));
            c1[3] = f_add(c1[3], f_mul(qc, l3b));
            /* l1 = mul, l2 = beta, l3 = L, l4 = R -> quartic */
            oF ma = f_mul(d[5], d[1]), mb = f_add(f_mul(d[5], b[1]), f_mul(b[5], d[1])), mc = f_mul(b[5], b[1]);
            oF ka = f_mul(ma, d[2]), kb = f_add(f_mul(ma, b[2]), f_mul(mb, d[2])), kc = f_add(f_mul(mb, b[2]), f_mul(mc, d[2])), kd = f_mul(mc, b[2]);
            c4[0] = f_add(c4[0], f_mul(ka, d[3]));
            c4[1] = f_add(c4[1], f_add(f_mul(ka, b[3]), f_mul(kb, d[3])));
            c4[2] = f_add(c4[2], f_add(f_mul(kb, b[3]), f_mul(kc, d[3])));
            c4[3] = f_add(c4[3], f_add(f_mul(kc, b[3]), f_mul(kd, d[3])));
            c4[4] = f_add(c4[4], f_mul(kd, b[3]));
            /* beta * O -> quadratic */
            c2[0] = f_add(c2[0], f_mul(d[1], d[4]));
            c2[1] = f_add(c2[1], f_add(f_mul(d[1], b[4]), f_mul(b[1], d[4])));
            c2[2] = f_add(c2[2], f_mul(b[1], b[4]));
        }
        oF p[5];
        p[0] = f_mul(a[2], c4[0]);
        p[1] = f_add(f_mul(a[2], c4[1]), c1[0]);
        p[2] = f_add(f_add(f_mul(a[2], c4[2]), c1[1]), f_mul(a[3], c2[0]));
        p[3] = f_add(f_add(f_mul(a[2], c4[3]), c1[2]), f_mul(a[3], c2[1]));
        p[4] = f_add(f_add(f_mul(a[2], c4[4]), c1[3]), f_mul(a[3], c2[2]));
        for (int q = 0; q < 5; q++) { rnd = mimc_hash(p[q], rnd); poly[5 * rd + q] = p[q]; }
        oF s01 = f_add(f_add(f_add(p[0], p[1]), f_add(p[2], p[3])), f_add(p[4], p[4]));      /* eval(0) + eval(1) */
        if (!(s01.re == sum.re && s01.im == sum.im)) *check = 0;
        sum = f_add(f_mul(f_add(f_mul(f_add(f_mul(f_add(f_mul(p[0], rnd), p[1]), rnd), p[2]), rnd), p[3]), rnd), p[4]);
        r[rd] = rnd;
        for (size_t j = 0; j < L; j++) for (int q = 0; q < 6; q++) t[q][j] = f_add(t[q][2 * j], f_mul(rnd, f_sub(t[q][2 * j + 1], t[q][2 * j])));
    }
    for (int q = 0; q < 6; q++) fin[q] = t[q][0];
    *rand_io = rnd; *sum_io = sum;
}
/* src/sumcheck.cpp:1974-2058: round i's tables are folded with the challenge that was current
 * BEFORE round i's polynomial is hashed (the fold sits in the same loop as the polynomial);
 * randomness[i] records that pre-round challenge.  v2-zero pairs contribute nothing; all-zero
 * pairs fold to zero (value-neutral shortcuts). */
void orc_sumcheck3(const oF *_v1, const oF *_v2, const oF *_v3, size_t n, const oF *prev_r, oF *cpoly, oF *r, oF *vr, oF *fin) {
    int rounds = (int)log2((double)n);
    oF *v1 = (oF *)malloc(sizeof(oF) * n), *v2 = (oF *)malloc(sizeof(oF) * n), *v3 = (oF *)malloc(sizeof(oF) * n);
    memcpy(v1, _v1, sizeof(oF) * n); memcpy(v2, _v2, sizeof(oF) * n); memcpy(v3, _v3, sizeof(oF) * n);
    oF rnd = *prev_r;
    for (int i = 0; i < rounds; i++) {
        size_t L = (size_t)1 << (rounds - 1 - i);
        oF pa = fint(0), pb = fint(0), pc = fint(0), pd = fint(0);
        for (size_t j = 0; j < L; j++) {
            if (!(fis0(v2[2 * j]) && fis0(v2[2 * j + 1]))) {
                oF a1 = f_sub(v1[2 * j + 1], v1[2 * j]), b1 = v1[2 * j];
                oF a2 = f_sub(v2[2 * j + 1], v2[2 * j]), b2 = v2[2 * j];
                oF a3 = f_sub(v3[2 * j + 1], v3[2 * j]), b3 = v3[2 * j];
                /* (l1*l2) = qa x^2 + qb x + qc ; then * l3 */
                oF qa = f_mul(a1, a2), qb = f_add(f_mul(a1, b2), f_mul(b1, a2)), qc = f_mul(b1, b2);
                pa = f_add(pa, f_mul(qa, a3));
                pb = f_add(pb, f_add(f_mul(qa, b3), f_mul(qb, a3)));
                pc = f_add(pc, f_add(f_mul(qb, b3), f_mul(qc, a3)));
                pd = f_add(pd, f_mul(qc, b3));
            }
            oF n1 = f_add(v1[2 * j], f_mul(rnd, f_sub(v1[2 * j + 1], v1[2 * j])));
            oF n2 = f_add(v2[2 * j], f_mul(rnd, f_sub(v2[2 * j + 1], v2[2 * j])));
            oF n3 = f_add(v3[2 * j], f_mul(rnd, f_sub(v3[2 * j + 1], v3[2 * j])));
            v1[j] = n1; v2[j] = n2; v3[j] = n3;
        }
        r[i] = rnd;
        rnd = mimc_hash(rnd, pa); rnd = mimc_hash(rnd, pb); rnd = mimc_hash(rnd, pc); rnd = mimc_hash(rnd, pd);
        cpoly[4 * i] = pa; cpoly[4 * i + 1] = pb; cpoly[4 * i + 2] = pc; cpoly[4 * i + 3] = pd;
    }
    rnd = mimc_hash(rnd, v1[0]); rnd = mimc_hash(rnd, v2[0]);
    vr[0] = v1[0]; vr[1] = v2[0]; vr[2] = v3[0]; *fin = rnd;
    free(v1); free(v2); free(v3);
}


/* ------------------------------------------------------------------------------------------ */
/* code-membership / FFT-as-sumcheck helpers                                                    */
/* ------------------------------------------------------------------------------------------ */
/* src/sumcheck.cpp:2888-2929: A = H^T beta over the expander graphs (lvl is passed by reference in
 * the reference; the recursive call gets a local copy l = lvl + R that is then discarded) */
static long long parity_rec(oF *A, const oF *beta, long long Offset, long long n, int dep, long long *lvl) {
    long long R = (long long)(k_alpha * n);
    if (n <= k_dist_thr) return n;
    const ograph *C = &gC[dep], *D = &gD[dep];
    for (long long i = 0; i < n; i++)
        for (int d = 0; d < C->degree; d++) {
            long long target = C->nbr[i * C->degree + d] + *lvl;
            A[i + Offset] = f_add(A[i + Offset], f_mul(beta[target], C->w[i * C->degree + d]));
        }
    for (long long i = 0; i < R; i++) A[i + Offset + n] = f_sub(A[i + Offset + n], beta[*lvl + i]);
    long long l = *lvl + R;
    long long L = parity_rec(A, beta, Offset + n, R, dep + 1, &l);
    R = D->R;
    for (long long i = 0; i < L; i++)
        for (int d = 0; d < D->degree; d++) {
            long long target = D->nbr[i * D->degree + d] + *lvl;
            A[i + Offset + n] = f_add(A[i + Offset + n], f_mul(beta[target], D->w[i * D->degree + d]));
        }
    for (long long i = 0; i < R; i++) A[i + Offset + n + L] = f_sub(A[i + Offset + n + L], beta[i + *lvl]);
    *lvl += R;
    return n + L + R;
}
/* A: size_a elements (zeroed here), beta: size_a elements */
long long orc_evaluate_parity_matrix(const oF *beta, size_t size_a, long long n, oF *A) {
    memset(A, 0, sizeof(oF) * size_a);
    long long lvl = 0;
    return parity_rec(A, beta, 0, n, 0, &lvl);
}
/* src/utils.cpp:676-755 phiPowInit + phiGInit; phi_g has 2^n entries, zero-initialised by the callers */
void orc_phi_g_init(const oF *rx, int n, const oF *scale, int is_ifft, oF *phi_g) {
    size_t N = (size_t)1 << n;
    oF *pm = (oF *)malloc(sizeof(oF) * N);
    oF phi = root_of_unity(n);
    if (is_ifft) phi = finv(phi);
    pm[0] = fint(1);
    for (size_t i = 1; i < N; i++) pm[i] = f_mul(pm[i - 1], phi);
    memset(phi_g, 0, sizeof(oF) * N);
    oF one = fint(1);
    if (is_ifft) {
        phi_g[0] = *scale; if (N > 1) phi_g[1] = *scale;
        for (int i = 1; i <= n; i++)
            for (size_t b = 0; b < ((size_t)1 << (i - 1)); b++) {
                size_t l = b, r = b ^ ((size_t)1 << (i - 1));
                int m = n - i;
                oF t1 = f_sub(one, rx[m]), t2 = f_mul(rx[m], pm[b << m]);
                phi_g[r] = f_mul(phi_g[l], f_sub(t1, t2));
                phi_g[l] = f_mul(phi_g[l], f_add(t1, t2));
            }
    } else {
        phi_g[0] = *scale;
        for (int i = 1; i < n; i++)
            for (size_t b = 0; b < ((size_t)1 << (i - 1)); b++) {
                size_t l = b, r = b ^ ((size_t)1 << (i - 1));
                int m = n - i;
                oF t1 = f_sub(one, rx[m]), t2 = f_mul(rx[m], pm[b << m]);
                phi_g[r] = f_mul(phi_g[l], f_sub(t1, t2));
                phi_g[l] = f_mul(phi_g[l], f_add(t1, t2));
            }
        for (size_t b = 0; b < ((size_t)1 << (n - 1)); b++) {
            oF t1 = f_sub(one, rx[0]), t2 = f_mul(rx[0], pm[b]);
            phi_g[b] = f_mul(phi_g[b], f_add(t1, t2));
        }
    }
    free(pm);
}
/* src/utils.cpp:758-775 prepare_matrix on a row-major rows x cols matrix: out[i] = fold of row i with r[0..k) */
void orc_prepare_matrix(const oF *M, size_t rows, size_t cols, const oF *r, int k, oF *out) {
    oF *row = (oF *)malloc(sizeof(oF) * cols);
    for (size_t i = 0; i < rows; i++) {
        memcpy(row, M + i * cols, sizeof(oF) * cols);
        size_t off = cols / 2;
        for (int t = 0; t < k; t++) {
            for (size_t j = 0; j < off; j++) row[j] = f_add(row[2 * j], f_mul(r[t], f_sub(row[2 * j + 1], row[2 * j])));
            off /= 2;
        }
        out[i] = row[0];
    }
    free(row);
}
/* src/sumcheck.cpp:3223-3235 prove_linear_code, with r1 given (the reference draws it with generate_randomness) */
void orc_prove_linear_code(const oF *codeword, size_t size, long long n, const oF *r1, oF *qpoly, oF *r, oF *vr, oF *fin) {
    int k = (int)log2((double)size);
    oF *beta = (oF *)malloc(sizeof(oF) * size), *A = (oF *)malloc(sizeof(oF) * size);
    orc_precompute_beta(r1, k, beta);
    orc_evaluate_parity_matrix(beta, size, n, A);
    orc_sumcheck2(A, codeword, size, &r1[k - 1], qpoly, r, vr, fin);
    free(beta); free(A);
}
/* src/sumcheck.cpp:2975-2987 prove_fft: m (size s) is zero-padded to 2s; r has log2(2s) entries */
void orc_prove_fft(const oF *m, size_t s, const oF *rr, oF *qpoly, oF *r, oF *vr, oF *fin) {
    size_t S = 2 * s; int k = (int)log2((double)S);
    oF *mm = (oF *)calloc(S, sizeof(oF)), *FG = (oF *)malloc(sizeof(oF) * S);
    memcpy(mm, m, sizeof(oF) * s);
    oF one = fint(1);
    orc_phi_g_init(rr, k, &one, 0, FG);
    orc_sumcheck2(FG, mm, S, &rr[k - 1], qpoly, r, vr, fin);
    free(mm); free(FG);
}
/* src/sumcheck.cpp:2989-3027 prove_fft_matrix: M rows x cols (row-major); columns zero-padded to 2 cols;
 * r = [r2 (log2(2cols)) | r1 (log2 rows)] */
void orc_prove_fft_matrix(const oF *M, size_t rows, size_t cols, const oF *rr, oF *qpoly, oF *r, oF *vr, oF *fin) {
    size_t C2 = 2 * cols; int k2 = (int)log2((double)C2), k1 = (int)log2((double)rows);
    /* transpose(M) padded: Mt[c][i] = M[i][c] (c < cols), 0 otherwise: C2 rows of `rows` elements */
    oF *Mt = (oF *)calloc(C2 * rows, sizeof(oF)), *arr = (oF *)malloc(sizeof(oF) * C2), *Fg = (oF *)malloc(sizeof(oF) * C2);
    for (size_t i = 0; i < rows; i++) for (size_t c = 0; c < cols; c++) Mt[c * rows + i] = M[i * cols + c];
    orc_prepare_matrix(Mt, C2, rows, rr + k2, k1, arr);
    oF one = fint(1);
    orc_phi_g_init(rr, k2, &one, 0, Fg);
    orc_sumcheck2(Fg, arr, C2, &rr[k1 + k2 - 1], qpoly, r, vr, fin);
    free(Mt); free(arr); free(Fg);
}

/* ------------------------------------------------------------------------------------------ */
/* inner PCS commitments of the opening: shockwave_commit (src/Virgo.cpp:120-157) and            */
/* whir_commit (:160-178) with change_form (:104-118)                                             */
/* ------------------------------------------------------------------------------------------ */
/* enc_out: k x (2N/k) row-major; levels_out: (2*(2N/k) - 1) hashes (column digests, then the tree) */
size_t orc_shockwave_commit(const oF *poly, size_t N, int k, oF *enc_out, uint8_t *levels_out) {
    size_t w = N / (size_t)k, W = 2 * w;
    int lg = (int)log2((double)W);
    for (int i = 0; i < k; i++) {
        oF *row = enc_out + (size_t)i * W; int nz = 0;
        memset(row, 0, sizeof(oF) * W);
        for (size_t j = 0; j < w; j++) { row[j] = poly[(size_t)i * w + j]; if (!fis0(row[j])) nz = 1; }
        if (nz) orc_fft(row, lg, 0);
    }
    oF *buff = (oF *)malloc(sizeof(oF) * (size_t)k);
    uint8_t *H = (uint8_t *)malloc(64 * (size_t)k);
    for (size_t c = 0; c < W; c++) {
        for (int j = 0; j < k; j++) buff[j] = enc_out[(size_t)j * W + c];
        size_t cnt = orc_mt_commit_blake(buff, (size_t)k, H);            /* column digest = root of the (quirky) tree over k/4 leaves */
        memcpy(levels_out + 32 * c, H + 32 * (cnt - 1), 32);
    }
    free(buff); free(H);
    return create_tree(levels_out, W);
}
static void change_form(oF *poly, int logn, int l, size_t pos, oF *buff) {
    size_t S = (size_t)1 << (logn - l);
    for (size_t i = 0; i < S / 2; i++) { buff[i] = poly[pos + 2 * i]; buff[i + S / 2] = f_sub(poly[pos + 2 * i + 1], poly[pos + 2 * i]); }
    memcpy(poly + pos, buff, sizeof(oF) * S);
    if (l + 1 == logn) return;
    change_form(poly, logn, l + 1, pos, buff);
    change_form(poly, logn, l + 1, pos + S / 2, buff);
}
void orc_change_form(oF *poly, int logn) { oF *b = (oF *)malloc(sizeof(oF) * ((size_t)1 << logn)); change_form(poly, logn, 0, 0, b); free(b); }
/* com_out: 2N F (poly_com after the permutation); levels_out: (2N/4)*2-1 hashes */
size_t orc_whir_commit(const oF *poly, size_t N, oF *com_out, uint8_t *levels_out) {
    int logn = (int)log2((double)N);
    size_t L = 2 * N;
    oF *pc = (oF *)calloc(L, sizeof(oF));
    memcpy(pc, poly, sizeof(oF) * N);
    orc_change_form(pc, logn);
    orc_fft(pc, logn + 1, 0);
    size_t q = L / 16, cnt = 0;
    for (size_t j = 0; j < q; j++) for (size_t kk = 0; kk < 16; kk++) com_out[cnt++] = pc[j + kk * q];
    free(pc);
    return orc_mt_commit_blake(com_out, L, levels_out);
}

/* ------------------------------------------------------------------------------------------ */
/* _whir_prove (src/Virgo.cpp:519-686) and shockwave_prove (:435-517), PROVER side only: the     */
/* verifier emulation inside them (_verify_iteration, MT_commit of replies, verify_claim_opt_     */
/* blake = SHA3) changes no prover state and draws nothing from libc, and is left out.  libc draws */
/* are made in the reference's order.  NOT pinned as a whole (the reference functions end in      */
/* SHA3 and cannot run in oracle/_ref); built from pinned pieces; the reference's own exit(-1)     */
/* checks ("Error in %d", "Error in final verification step") are evaluated into `checks`.        */
/* ------------------------------------------------------------------------------------------ */
static void compute_zetas(oF *z /* [reps][v] */, int reps, int v, size_t Nq, int32_t *ridx /* reps-1 or NULL */) {   /* src/Virgo.cpp:220-236 */
    z[0] = fint((uint64_t)random());
    oF omega = root_of_unity((int)log2((double)Nq));
    for (int i = 1; i < reps; i++) {
        long rr = rand() % (long)Nq;
        if (ridx) ridx[i - 1] = (int32_t)rr;
        u128 e = (u128)rr;
        oF ret = fint(1), tmp = omega;
        while (e) { if (e & 1) ret = f_mul(ret, tmp); tmp = f_mul(tmp, tmp); e >>= 1; }
        z[(size_t)i * v] = ret;
    }
    for (int i = 0; i < reps; i++) for (int j = 1; j < v; j++) z[(size_t)i * v + j] = f_mul(z[(size_t)i * v + j - 1], z[(size_t)i * v + j - 1]);
}
static void whir_answer(orc_whir_queries *Q, const oF *layer /* regrouped */, const uint8_t *levels, size_t size, const int32_t *ridx, int n,
                        size_t *q_tot, size_t *path_off, int round_t) {
    int depth = (int)log2((double)(size / 4));
    for (int i = 0; i < n; i++) {
        size_t q = *q_tot + (size_t)i;
        if (Q->qidx) Q->qidx[q] = ridx[i];
        if (Q->qreply) memcpy(Q->qreply + 16 * q, layer + 16 * (size_t)ridx[i], 16 * sizeof(oF));
        if (Q->qpaths) { orc_open_tree_blake(levels, size / 4, (size_t)ridx[i], 0, 0, Q->qpaths + *path_off); }
        *path_off += 32 * (size_t)depth;
    }
    *q_tot += (size_t)n;
    if (Q->nq) Q->nq[round_t] = n;
}
/* outputs: qpoly (3 per fold round, all iterations back to back), a_out (the libc fold challenges), fri_roots (32 B per
 * iteration), scal = {final eval, final sum}; checks[0] = all round sums matched, checks[1] = final sum == eval.
 * Returns the number of iterations. */
/* Query material of _verify_iteration (src/Virgo.cpp:245-275), which the prover assembles: round t = 1..iters answers
 * R_t - 1 indices r (compute_zetas' rand() % Nq draws) against the PREVIOUS layer (t = 1: the whir_commit codeword `com`
 * (regrouped, as orc_whir_commit returns it) and its tree; t >= 2: FRI layer t-1): reply = the 16 elements
 * layer[r + j*size/16] = regrouped[16 r + j], path = open_tree_blake(tree, {r, 0}, 0) (leaf r: the reference opens leaf r,
 * not the four leaves that hold the 16 reply elements -- kept).  Q->qidx / qreply (16 per query) / qpaths (depth_t x 32 B per
 * query, back to back; depth_t = log2(size_t / 4)) / final_pb (final_poly | final_beta, `remaining` each) / nq[t-1] per round. */
int orc_whir_prove_ex(const oF *poly_in, size_t N, const oF *x, const oF *com, const uint8_t *com_levels, oF *qpoly, oF *a_out, uint8_t *fri_roots,
                      oF *scal, int *checks, orc_whir_queries *Q) {
    const int k = 4, logN = (int)log2((double)N);
    const oF *prev = com; const uint8_t *prev_lv = com_levels; size_t prev_sz = 2 * N;     /* layer the next query round reads */
    oF *keep_buf = NULL; uint8_t *keep_lv = NULL;
    size_t q_tot = 0, path_off = 0; int round_t = 0;
    oF *poly = (oF *)malloc(sizeof(oF) * N), *beta = (oF *)malloc(sizeof(oF) * N);
    memcpy(poly, poly_in, sizeof(oF) * N);
    orc_precompute_beta(x, logN, beta);
    oF eval = fint(0);
    for (size_t i = 0; i < N; i++) eval = f_add(eval, f_mul(beta[i], poly[i]));
    int iter = 0, repeats = 100, nq = 0; size_t remaining = 0;
    checks[0] = 1; checks[1] = 0;
    for (;;) {
        for (int i = 0; i < k; i++) {
            size_t L = N >> (iter * k + i + 1);
            oF pa = fint(0), pb = fint(0), pc = fint(0);
            for (size_t j = 0; j < L; j++) {
                oF d1 = f_sub(poly[j + L], poly[j]), d2 = f_sub(beta[j + L], beta[j]);
                pa = f_add(pa, f_mul(d1, d2)); pb = f_add(pb, f_add(f_mul(d1, beta[j]), f_mul(poly[j], d2))); pc = f_add(pc, f_mul(poly[j], beta[j]));
            }
            oF a = fint((uint64_t)random());
            oF s01 = f_add(f_add(pa, pb), f_add(pc, pc));
            if (!(s01.re == eval.re && s01.im == eval.im)) checks[0] = 0;
            eval = f_add(f_mul(f_add(f_mul(pa, a), pb), a), pc);
            qpoly[3 * nq] = pa; qpoly[3 * nq + 1] = pb; qpoly[3 * nq + 2] = pc; a_out[nq] = a; nq++;
            for (size_t j = 0; j < L; j++) { poly[j] = f_add(poly[j], f_mul(a, f_sub(poly[j + L], poly[j]))); beta[j] = f_add(beta[j], f_mul(a, f_sub(beta[j + L], beta[j]))); }
        }
        iter++;
        size_t cur = N >> (k * iter), fsz = (2 * N) >> iter;
        oF *fp = (oF *)calloc(fsz, sizeof(oF)), *buff = (oF *)malloc(sizeof(oF) * fsz);
        memcpy(fp, poly, sizeof(oF) * cur);
        orc_change_form(fp, (int)log2((double)cur));
        orc_fft(fp, (int)log2((double)fsz), 0);
        int queries = (int)(100.0 / log2((double)fsz / (double)cur));
        size_t q16 = fsz / 16, cnt = 0;
        for (size_t i = 0; i < q16; i++) for (size_t j = 0; j < 16; j++) buff[cnt++] = fp[i + j * q16];
        uint8_t *lv = (uint8_t *)malloc(32 * (fsz / 2));
        size_t nl = orc_mt_commit_blake(buff, fsz, lv);
        memcpy(fri_roots + 32 * (iter - 1), lv + 32 * (nl - 1), 32);
        free(fp);
        if (logN - iter * k <= k) { repeats = queries; remaining = (size_t)1 << (logN - iter * k); free(lv); free(buff); break; }
        int v = logN - iter * k;
        oF *z = (oF *)malloc(sizeof(oF) * (size_t)repeats * v), *y = (oF *)malloc(sizeof(oF) * (size_t)repeats), *_b = (oF *)malloc(sizeof(oF) * cur);
        int32_t *ridx = (int32_t *)malloc(sizeof(int32_t) * (size_t)repeats);
        compute_zetas(z, repeats, v, (2 * N) >> (iter + k), ridx);
        for (int i = 0; i < repeats; i++) {
            orc_precompute_beta(z + (size_t)i * v, v, _b);
            oF acc = fint(0);
            for (size_t j = 0; j < cur; j++) acc = f_add(acc, f_mul(_b[j], poly[j]));
            y[i] = acc;
        }
        oF sch = fint((uint64_t)random()), pw = sch;
        for (int i = 0; i < repeats; i++) {
            orc_precompute_beta(z + (size_t)i * v, v, _b);
            for (size_t j = 0; j < cur; j++) beta[j] = f_add(beta[j], f_mul(pw, _b[j]));
            eval = f_add(eval, f_mul(pw, y[i]));
            pw = f_mul(pw, sch);
        }
        free(z); free(y); free(_b);
        /* _verify_iteration(data, a, r, repeats, iter): replies and paths against the previous layer */
        if (Q && prev) whir_answer(Q, prev, prev_lv, prev_sz, ridx, repeats - 1, &q_tot, &path_off, round_t);
        round_t++;
        free(ridx);
        free(keep_buf); free(keep_lv); keep_buf = buff; keep_lv = lv; prev = buff; prev_lv = lv; prev_sz = fsz;
        repeats = queries;
    }
    oF sum = fint(0);
    for (size_t i = 0; i < remaining; i++) sum = f_add(sum, f_mul(poly[i], beta[i]));
    checks[1] = (sum.re == eval.re && sum.im == eval.im);
    scal[0] = eval; scal[1] = sum;
    /* closing draws (src/Virgo.cpp:652-655): generate_randomness(log2 remaining) and one more compute_zetas, kept so that
     * the libc stream after this call is where the reference leaves it */
    {
        int lr = (int)log2((double)remaining);
        oF *a2 = (oF *)malloc(sizeof(oF) * (size_t)(lr + 1)); orc_generate_randomness(lr, a2); free(a2);
        oF *z = (oF *)malloc(sizeof(oF) * (size_t)repeats * (size_t)(lr > 0 ? lr : 1));
        int32_t *ridx = (int32_t *)malloc(sizeof(int32_t) * (size_t)(repeats + 1));
        if (repeats > 0 && lr > 0) {
            compute_zetas(z, repeats, lr, (2 * N) >> (iter * k), ridx);
            if (Q && prev) whir_answer(Q, prev, prev_lv, prev_sz, ridx, repeats - 1, &q_tot, &path_off, round_t);
        }
        free(z); free(ridx);
    }
    if (Q && Q->final_pb) { memcpy(Q->final_pb, poly, sizeof(oF) * remaining); memcpy(Q->final_pb + remaining, beta, sizeof(oF) * remaining); }
    free(keep_buf); free(keep_lv);
    free(poly); free(beta);
    return iter;
}
int orc_whir_prove(const oF *poly_in, size_t N, const oF *x, oF *qpoly, oF *a_out, uint8_t *fri_roots, oF *scal, int *checks) {
    return orc_whir_prove_ex(poly_in, N, x, NULL, NULL, qpoly, a_out, fri_roots, scal, checks, NULL);
}
/* matrix: k x w (the committed polynomial, row-major), enc: k x 2w; x: challenge vector (its last log2 k entries pick the rows).
 * P1/P2 transcripts as sumcheck2 (P1: log2(2w) rounds, P2: log2(2w) rounds), whir outputs as orc_whir_prove, I_out: 240 indices. */
/* _ex: also the 240 query replies (k F each: column I[i] of enc) and, given the commitment's tree `levels` (as
 * orc_shockwave_commit returns it), their paths open_tree_blake(MT, {I[i], 0}, 0) (src/Virgo.cpp:468-472, 503-504), log2(2w) x 32 B
 * each; plus the WHIR query material (orc_whir_prove_ex). */
int orc_shockwave_prove_ex(const oF *matrix, const oF *enc, const uint8_t *levels, size_t N, int k, const oF *x, int xlen, uint32_t *I_out, oF *q1, oF *r1o, oF *vr1,
                           oF *fin1, oF *q2, oF *r2o, oF *vr2, oF *fin2, oF *wq, oF *wa, uint8_t *wroots, oF *wscal, int *wchecks, uint8_t *whir_root,
                           oF *reply, uint8_t *paths, orc_whir_queries *Q) {
    size_t w = N / (size_t)k, W = 2 * w; int lk = (int)log2((double)k), lgW = (int)log2((double)W);
    oF *beta1 = (oF *)malloc(sizeof(oF) * (size_t)k), *aggr = (oF *)calloc(w, sizeof(oF)), *at = (oF *)calloc(W, sizeof(oF));
    orc_precompute_beta(x + xlen - lk, lk, beta1);
    for (size_t i = 0; i < W; i++) {
        if (i < w) for (int j = 0; j < k; j++) aggr[i] = f_add(aggr[i], f_mul(beta1[j], matrix[(size_t)j * w + i]));
        for (int j = 0; j < k; j++) at[i] = f_add(at[i], f_mul(beta1[j], enc[(size_t)j * W + i]));
    }
    oF *com = NULL; uint8_t *clv = NULL;
    if (w > 256) { com = (oF *)malloc(sizeof(oF) * 2 * w); clv = (uint8_t *)malloc(32 * w); size_t c = orc_whir_commit(aggr, w, com, clv); memcpy(whir_root, clv + 32 * (c - 1), 32); }
    oF *buff1 = (oF *)calloc(W, sizeof(oF));
    for (int i = 0; i < 240; i++) { I_out[i] = (uint32_t)(rand() % (long)W); }
    for (int i = 0; i < 240; i++) {
        if (reply) for (int j = 0; j < k; j++) reply[(size_t)i * k + j] = enc[(size_t)j * W + I_out[i]];
        if (paths && levels) orc_open_tree_blake(levels, W, I_out[i], 0, 0, paths + (size_t)i * 32 * (size_t)lgW);
    }
    for (int i = 0; i < 240; i++) buff1[I_out[i]] = fint(1);
    oF p33 = fint(33);
    orc_sumcheck2(at, buff1, W, &p33, q1, r1o, vr1, fin1);
    orc_prove_fft(aggr, w, r1o, q2, r2o, vr2, fin2);                 /* prove_fft(aggr, P1.randomness[0], P1.vr[0]) */
    int iters = 0;
    /* src/Virgo.cpp:479 tests aggr.size()/2 > 256 AFTER prove_fft, which takes its vector by reference and doubles it
       (src/sumcheck.cpp:2984-2985): the test is on the original width w, the same as whir_commit's (:458) */
    if (w > 256) iters = orc_whir_prove_ex(aggr, w, r2o, com, clv, wq, wa, wroots, wscal, wchecks, Q);   /* x = P2.randomness[0] minus its last entry: log2 w entries */
    free(beta1); free(aggr); free(at); free(buff1); free(com); free(clv);
    return iters;
}
int orc_shockwave_prove(const oF *matrix, const oF *enc, size_t N, int k, const oF *x, int xlen, uint32_t *I_out, oF *q1, oF *r1o, oF *vr1, oF *fin1,
                        oF *q2, oF *r2o, oF *vr2, oF *fin2, oF *wq, oF *wa, uint8_t *wroots, oF *wscal, int *wchecks, uint8_t *whir_root) {
    return orc_shockwave_prove_ex(matrix, enc, NULL, N, k, x, xlen, I_out, q1, r1o, vr1, fin1, q2, r2o, vr2, fin2, wq, wa, wroots, wscal, wchecks, whir_root, NULL, NULL, NULL);
}

/* ------------------------------------------------------------------------------------------ */
/* batch_3product_sumcheck (src/sumcheck.cpp:275-372): cubic sumcheck over `batches` table       */
/* triples of different power-of-two lengths with coefficients a[j]; hash first, then fold;      */
/* a triple already folded to one element contributes (-x t + x)^3-style terms and folds by      */
/* (1 - rand).  Tables are passed concatenated (lens[j] elements each) and folded in place.      */
/* vr: 3*batches F (the values when a triple first reaches length 1, else the final elements).   */
/* ------------------------------------------------------------------------------------------ */
static void cubic_of(oF x0, oF x1, oF y0, oF y1, oF z0, oF z1, oF *p) {   /* p[0..3] += (l1*l2)*l3 coefficients */
    oF dx = f_sub(x1, x0), dy = f_sub(y1, y0), dz = f_sub(z1, z0);
    oF qa = f_mul(dx, dy), qb = f_add(f_mul(dx, y0), f_mul(x0, dy)), qc = f_mul(x0, y0);
    p[0] = f_add(p[0], f_mul(qa, dz));
    p[1] = f_add(p[1], f_add(f_mul(qa, z0), f_mul(qb, dz)));
    p[2] = f_add(p[2], f_add(f_mul(qb, z0), f_mul(qc, dz)));
    p[3] = f_add(p[3], f_mul(qc, z0));
}
int orc_batch_3product_sumcheck(oF *t1, oF *t2, oF *t3, const size_t *lens, int batches, const oF *a, oF *cpoly, oF *r_out, oF *vr) {
    size_t Lmax = 0;
    for (int j = 0; j < batches; j++) if (lens[j] > Lmax) Lmax = lens[j];
    int rounds = (int)log2((double)Lmax);
    oF rnd = fint(312);
    size_t *off = (size_t *)malloc(sizeof(size_t) * (size_t)batches);
    char *set = (char *)calloc((size_t)batches, 1);
    size_t o = 0; for (int j = 0; j < batches; j++) { off[j] = o; o += lens[j]; }
    for (int i = 0; i < rounds; i++) {
        oF poly[4] = {fint(0), fint(0), fint(0), fint(0)};
        for (int j = 0; j < batches; j++) {
            oF *x = t1 + off[j], *y = t2 + off[j], *z = t3 + off[j];
            int lg = (int)log2((double)lens[j]);
            size_t L = (lg - 1 - i >= 0) ? ((size_t)1 << (lg - 1 - i)) : 0;
            oF p[4] = {fint(0), fint(0), fint(0), fint(0)};
            if (L >= 1) { for (size_t k = 0; k < L; k++) cubic_of(x[2 * k], x[2 * k + 1], y[2 * k], y[2 * k + 1], z[2 * k], z[2 * k + 1], p); }
            else {
                if (!set[j]) { vr[3 * j] = x[0]; vr[3 * j + 1] = y[0]; vr[3 * j + 2] = z[0]; set[j] = 1; }
                cubic_of(x[0], fint(0), y[0], fint(0), z[0], fint(0), p);       /* linear_poly(-v, v): value v at 0, 0 at 1 */
            }
            for (int q = 0; q < 4; q++) poly[q] = f_add(poly[q], f_mul(a[j], p[q]));
        }
        for (int q = 0; q < 4; q++) { rnd = mimc_hash(rnd, poly[q]); cpoly[4 * i + q] = poly[q]; }
        r_out[i] = rnd;
        for (int j = 0; j < batches; j++) {
            oF *x = t1 + off[j], *y = t2 + off[j], *z = t3 + off[j];
            int lg = (int)log2((double)lens[j]);
            size_t L = (lg - 1 - i >= 0) ? ((size_t)1 << (lg - 1 - i)) : 0;
            if (L >= 1) for (size_t k = 0; k < L; k++) {
                x[k] = f_add(x[2 * k], f_mul(rnd, f_sub(x[2 * k + 1], x[2 * k])));
                y[k] = f_add(y[2 * k], f_mul(rnd, f_sub(y[2 * k + 1], y[2 * k])));
                z[k] = f_add(z[2 * k], f_mul(rnd, f_sub(z[2 * k + 1], z[2 * k])));
            } else {
                oF om = f_sub(fint(1), rnd);
                x[0] = f_mul(om, x[0]); y[0] = f_mul(om, y[0]); z[0] = f_mul(om, z[0]);
            }
        }
    }
    for (int j = 0; j < batches; j++) if (!set[j]) { vr[3 * j] = t1[off[j]]; vr[3 * j + 1] = t2[off[j]]; vr[3 * j + 2] = t3[off[j]]; }
    free(off); free(set);
    return rounds;
}

/* ------------------------------------------------------------------------------------------ */
/* prove_multiplication_tree_new (src/sumcheck.cpp:35-257) for power-of-two `vectors` x `size`     */
/* inputs (the reference pads otherwise).  prev_x: NULL -> the reference draws                   */
/* generate_randomness(log2 vectors) (vectors > 1).  Layer proofs are written back to back from   */
/* the top layer (depth-1) down to layer 0: cpoly (4 per round), r, and per layer vr[3], fin.     */
/* final_r has log2(vectors*size) entries.  Returns the number of sumcheck layers written.       */
/* ------------------------------------------------------------------------------------------ */
int orc_mul_tree(const oF *input, size_t vectors, size_t size, const oF *previous_r_in, const oF *prev_x, oF *cpoly, oF *r_out, oF *vr, oF *fin,
                 oF *final_r, oF *out_eval, oF *final_eval) {
    size_t total = vectors * size;
    int depth = (int)log2((double)size), lt = (int)log2((double)total);
    oF **tr = (oF **)malloc(sizeof(oF *) * (size_t)depth), **in1 = (oF **)malloc(sizeof(oF *) * (size_t)depth), **in2 = (oF **)malloc(sizeof(oF *) * (size_t)depth);
    const oF *src = input; size_t len = total;
    for (int i = 0; i < depth; i++) {
        len /= 2;
        tr[i] = (oF *)malloc(sizeof(oF) * len); in1[i] = (oF *)malloc(sizeof(oF) * len); in2[i] = (oF *)malloc(sizeof(oF) * len);
        for (size_t j = 0; j < len; j++) { in1[i][j] = src[2 * j]; in2[i][j] = src[2 * j + 1]; tr[i][j] = f_mul(src[2 * j], src[2 * j + 1]); }
        src = tr[i];
    }
    oF previous_r = *previous_r_in, sum;
    oF *r = (oF *)malloc(sizeof(oF) * (size_t)(lt + 1)); int rl = 0, layers = 0;
    size_t qo = 0, ro = 0;
    if (vectors == 1) {
        previous_r = mimc_hash(previous_r, tr[depth - 1][0]);
        sum = tr[depth - 1][0]; *out_eval = sum;
    } else {
        rl = (int)log2((double)vectors);
        if (prev_x) memcpy(r, prev_x, sizeof(oF) * (size_t)rl); else orc_generate_randomness(rl, r);
        orc_evaluate_vector(tr[depth - 1], vectors, r, rl, &sum); *out_eval = sum;
        if (!prev_x) previous_r = mimc_hash(r[rl - 1], sum);
    }
    for (int i = depth - 1; i >= 0; i--) {
        if (rl == 0) {
            oF num = mimc_hash(previous_r, in1[i][0]);
            previous_r = mimc_hash(num, in2[i][0]);
            sum = f_add(f_mul(f_sub(fint(1), previous_r), in1[i][0]), f_mul(previous_r, in2[i][0]));
            r[rl++] = previous_r;
        } else {
            size_t n = (size_t)1 << rl;
            oF *beta = (oF *)malloc(sizeof(oF) * n);
            orc_precompute_beta(r, rl, beta);
            orc_sumcheck3(in1[i], in2[i], beta, n, &previous_r, cpoly + qo, r_out + ro, vr + 3 * layers, fin + layers);
            free(beta);
            memcpy(r + 1, r_out + ro, sizeof(oF) * (size_t)rl);          /* r = P.randomness[0]; r.insert(begin, previous_r) */
            previous_r = fin[layers];
            sum = f_add(f_mul(vr[3 * layers], f_sub(fint(1), previous_r)), f_mul(vr[3 * layers + 1], previous_r));
            r[0] = previous_r;
            qo += 4 * (size_t)rl; ro += (size_t)rl; rl++; layers++;
        }
    }
    memcpy(final_r, r, sizeof(oF) * (size_t)rl); *final_eval = sum;
    for (int i = 0; i < depth; i++) { free(tr[i]); free(in1[i]); free(in2[i]); }
    free(tr); free(in1); free(in2); free(r);
    return layers;
}

/* ------------------------------------------------------------------------------------------ */
/* streaming-sumcheck error terms and folds (the per-chunk work of HOBBIT's space-efficient      */
/* sumchecks): src/sumcheck.cpp:374-432 (compute{2,3,4}p_error_terms, has_lookups == false),      */
/* 1093-1136 (batch_prod), 862-869 (fold += rand * chunk)                                         */
/* ------------------------------------------------------------------------------------------ */
/* has_lookups / lookup_rand[0..1] (src/main.cpp:67,70): the gate maps of compute{3,4}p_error_terms when set (:388-394, :413-427) */
static int g_has_lookups = 0; static oF g_lookup_rand[2];
void orc_set_lookups(int on, const oF *lr) { g_has_lookups = on; if (on) { g_lookup_rand[0] = lr[0]; g_lookup_rand[1] = lr[1]; } }
static oF lk_gate3(int s, const oF *lr) { return s == 0 ? fint(1) : s == 2 ? lr[0] : s == 3 ? lr[1] : s == 4 ? fint(1) : fint(0); }
void orc_err2p(const oF *b1, const oF *b2, const oF *f1, const oF *f2, size_t n, oF *K) {
    for (size_t i = 0; i < n; i++) {
        K[0] = f_add(K[0], f_add(f_mul(b1[i], f2[i]), f_mul(b2[i], f1[i])));
        K[1] = f_add(K[1], f_mul(b1[i], b2[i]));
    }
}
void orc_err3p(const oF *b1, const int32_t *b2, const oF *f1, const oF *f2, const oF *f3, const oF *beta, size_t n, oF *K) {
    for (size_t j = 0; j < n; j++) {
        oF gate = g_has_lookups ? lk_gate3(b2[j], g_lookup_rand) : fint((uint64_t)(int64_t)b2[j]);      /* F(buff2[j]), selectors are 0/1 without lookups */
        oF t1 = f_add(f_mul(b1[j], f2[j]), f_mul(gate, f1[j]));
        oF t2 = f_mul(b1[j], gate);
        K[0] = f_add(K[0], f_add(f_mul(f3[j], t1), f_mul(f_mul(beta[j], f1[j]), f2[j])));
        K[1] = f_add(K[1], f_add(f_mul(beta[j], t1), f_mul(f3[j], t2)));
        K[2] = f_add(K[2], f_mul(t2, beta[j]));
    }
}
void orc_err4p(const oF *b1, const oF *b2, const oF *b3, const int32_t *b4, const oF *f1, const oF *f2, const oF *f3, const oF *f4, size_t n, oF *K) {
    for (size_t i = 0; i < n; i++) {
        oF gate = g_has_lookups ? fint(b4[i] == 1 ? 1 : 0) : f_sub(fint(1), fint((uint64_t)(int64_t)b4[i]));
        oF t1 = f_add(f_mul(f1[i], b2[i]), f_mul(f2[i], b1[i]));
        oF t2 = f_add(f_mul(f3[i], gate), f_mul(f4[i], b3[i]));
        oF t3 = f_mul(b1[i], b2[i]), t4 = f_mul(gate, b3[i]), t5 = f_mul(f1[i], f2[i]), t6 = f_mul(f3[i], f4[i]);
        K[0] = f_add(K[0], f_add(f_mul(t1, t6), f_mul(t2, t5)));
        K[1] = f_add(K[1], f_add(f_add(f_mul(t1, t2), f_mul(t3, t6)), f_mul(t4, t5)));
        K[2] = f_add(K[2], f_add(f_mul(t1, t4), f_mul(t2, t3)));
        K[3] = f_add(K[3], f_mul(t3, t4));
    }
}
/* one batch of batch_prod's error terms: K[0..2] += (K1_temp, K2_temp, K3[j]) */
void orc_batch_prod_terms(const oF *b1, const oF *b2, const oF *b3, const oF *f1, const oF *f2, const oF *f3, size_t n, oF *K) {
    for (size_t k = 0; k < n; k++) {
        oF t1 = f_add(f_mul(b1[k], f2[k]), f_mul(b2[k], f1[k])), t2 = f_mul(b1[k], b2[k]);
        K[0] = f_add(K[0], f_add(f_mul(f3[k], t1), f_mul(f_mul(b3[k], f1[k]), f2[k])));
        K[1] = f_add(K[1], f_add(f_mul(b3[k], t1), f_mul(f3[k], t2)));
        K[2] = f_add(K[2], f_mul(t2, b3[k]));
    }
}
void orc_fold_axpy(oF *fold, const oF *buff, const oF *rnd, size_t n) { for (size_t i = 0; i < n; i++) fold[i] = f_add(fold[i], f_mul(*rnd, buff[i])); }

/* batch_prod (src/sumcheck.cpp:1093-1136), one step: tables flat [batches][n]; r_last = R.back(); remaining_betas[j][i] given per
 * batch; Kf / K_partial accumulated; the three fold tables updated in place; returns the new challenge */
void orc_batch_prod(oF *f1, oF *f2, oF *f3, const oF *b1, const oF *b2, const oF *b3, int batches, size_t n, const oF *r_last, const oF *a,
                    const oF *rem_beta, oF *Kf, oF *Kp, oF *rand_out) {
    oF K1 = fint(0), K2 = fint(0);
    oF *K3 = (oF *)calloc((size_t)batches, sizeof(oF));
    for (int j = 0; j < batches; j++) {
        oF K[3] = {fint(0), fint(0), fint(0)};
        orc_batch_prod_terms(b1 + (size_t)j * n, b2 + (size_t)j * n, b3 + (size_t)j * n, f1 + (size_t)j * n, f2 + (size_t)j * n, f3 + (size_t)j * n, n, K);
        K1 = f_add(K1, f_mul(a[j], K[0])); K2 = f_add(K2, f_mul(a[j], K[1])); K3[j] = K[2];
    }
    oF rnd = mimc_hash(K1, *r_last);                       /* note the argument order: mimc_hash(K, rand) */
    rnd = mimc_hash(K2, rnd);
    for (int j = 0; j < batches; j++) rnd = mimc_hash(K3[j], rnd);
    oF x1 = rnd, x2 = f_mul(rnd, x1), x3 = f_mul(rnd, x2);
    for (int j = 0; j < batches; j++) {
        Kp[j] = f_add(Kp[j], f_mul(rem_beta[j], K3[j]));
        *Kf = f_add(*Kf, f_mul(f_mul(x3, a[j]), K3[j]));
    }
    *Kf = f_add(*Kf, f_add(f_mul(x2, K2), f_mul(x1, K1)));
    *rand_out = rnd;
    size_t tot = (size_t)batches * n;
    orc_fold_axpy(f1, b1, &rnd, tot); orc_fold_axpy(f2, b2, &rnd, tot); orc_fold_axpy(f3, b3, &rnd, tot);
    free(K3);
}

/* ------------------------------------------------------------------------------------------ */
/* Our_PC open, "core" = open_standard (src/Our_PC.cpp:604-661) + recursive_prover_Spielman       */
/* (src/PC_utils.cpp:271-385) WITHOUT the inner shockwave/WHIR commitments and proofs             */
/* (shockwave_commit in _aggregate, the two shockwave_prove calls).  The libc draws follow the   */
/* reference's order up to the first shockwave_prove, so P1..P5 are what the reference computes. */
/* NOT pinned as a whole against oracle/_ref (the reference's open path ends in SHA3 from the     */
/* prebuilt libXKCP.a and cannot run); every primitive used here is pinned individually, and the */
/* reference's own consistency checks ("Error recursion 1/2", prove_fft_matrix's sum check) are   */
/* evaluated and returned in `checks`.                                                            */
/* ------------------------------------------------------------------------------------------ */
static void matvec_rows(const oF *Mx, size_t rows, size_t cols, const oF *v, oF *out) {   /* out[i] = sum_j v[j] M[i][j] */
    for (size_t i = 0; i < rows; i++) { oF a = fint(0); for (size_t j = 0; j < cols; j++) a = f_add(a, f_mul(v[j], Mx[i * cols + j])); out[i] = a; }
}
/* aggr_in != NULL: the aggregate is given (multi-GPU open: it was summed from per-rank partials); poly / x are then unused */
static int open_core_impl(const oF *aggr_in, const oF *poly, size_t N, int K, int trs, const oF *x, int queries, uint32_t *I_out, oF *reply_out, const oF *tensor,
                          oF *scalars_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, uint8_t *roots);
int orc_open_core(const oF *poly, size_t N, int K, int trs, const oF *x, int queries, uint32_t *I_out, oF *reply_out, const oF *tensor /* K x 2trs x cols, row-major */,
                  oF *scalars_out /* r_v0, s0, s2, a, y1 */, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, uint8_t *roots /* C_f, C_c (64 B) or NULL */) {
    return open_core_impl(NULL, poly, N, K, trs, x, queries, I_out, reply_out, tensor, scalars_out, qpoly, r_out, vr, fin, checks, roots);
}
int orc_open_core_aggr(const oF *aggr, size_t M, int K, int trs, int queries, uint32_t *I_out, oF *scalars_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks,
                       uint8_t *roots) {
    return open_core_impl(aggr, NULL, M * (size_t)K, K, trs, NULL, queries, I_out, NULL, NULL, scalars_out, qpoly, r_out, vr, fin, checks, roots);
}
static int open_core_impl(const oF *aggr_in, const oF *poly, size_t N, int K, int trs, const oF *x, int queries, uint32_t *I_out, oF *reply_out, const oF *tensor,
                          oF *scalars_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, uint8_t *roots) {
    size_t M = N / (size_t)K, cols = 2 * M / (size_t)trs, rows2 = 2 * (size_t)trs;
    int logK = (int)log2((double)K), logc = (int)log2((double)cols), R1 = (int)log2((double)rows2);
    /* open_standard: beta over the chunk variables, r_v[0] draw, aggregate */
    oF *beta = (oF *)malloc(sizeof(oF) * (size_t)K);
    if (!aggr_in) orc_precompute_beta(x, logK, beta);
    oF rv0; orc_generate_randomness(1, &rv0); scalars_out[0] = rv0;
    oF *aggr = (oF *)malloc(sizeof(oF) * M);
    if (aggr_in) memcpy(aggr, aggr_in, sizeof(oF) * M); else orc_aggregate(poly, N, beta, K, aggr);
    /* compute_tensorcode(aggr): message half M' (row FFT) and parity half C */
    oF *T = (oF *)malloc(sizeof(oF) * rows2 * cols);
    orc_compute_tensorcode(aggr, M, trs, 1, T);
    const oF *C = T + (size_t)trs * cols;
    if (roots) {   /* _aggregate's inner commitments (src/Our_PC.cpp:274-287): C_f over aggr, C_c over the parity half, 32 rows each */
        size_t nf = M, nc = (size_t)trs * cols;
        oF *enc = (oF *)malloc(sizeof(oF) * 2 * (nf > nc ? nf : nc));
        uint8_t *lv = (uint8_t *)malloc(64 * (2 * (nf > nc ? nf : nc) / 32) * 2);
        size_t cnt = orc_shockwave_commit(aggr, nf, 32, enc, lv); memcpy(roots, lv + 32 * (cnt - 1), 32);
        cnt = orc_shockwave_commit(C, nc, 32, enc, lv); memcpy(roots + 32, lv + 32 * (cnt - 1), 32);
        free(enc); free(lv);
    }
    oF *Mp = (oF *)calloc((size_t)trs * cols, sizeof(oF));
    for (size_t i = 0; i < (size_t)trs; i++) { memcpy(Mp + i * cols, aggr + i * (cols / 2), sizeof(oF) * (cols / 2)); orc_fft(Mp + i * cols, logc, 0); }
    /* queries (src/Our_PC.cpp:633-641) and replies */
    size_t *Iv = (size_t *)malloc(sizeof(size_t) * (size_t)queries);
    for (int q = 0; q < queries; q++) {
        uint32_t c = (uint32_t)(rand() % (long)cols), rw = (uint32_t)(rand() % (long)rows2);
        I_out[2 * q] = c; I_out[2 * q + 1] = rw; Iv[q] = c + cols * (size_t)rw;
        if (tensor && reply_out) for (int i = 0; i < K; i++) reply_out[(size_t)q * K + i] = tensor[((size_t)i * rows2 + rw) * cols + c];
    }
    /* recursive_prover_Spielman */
    oF *sv = (oF *)malloc(sizeof(oF) * cols);
    sv[0] = fint((uint64_t)random()); scalars_out[1] = sv[0];
    for (size_t i = 1; i < cols; i++) sv[i] = f_mul(sv[i - 1], sv[0]);
    oF *aggr_c = (oF *)malloc(sizeof(oF) * rows2);
    matvec_rows(Mp, trs, cols, sv, aggr_c); matvec_rows(C, trs, cols, sv, aggr_c + trs);
    oF *r1 = (oF *)malloc(sizeof(oF) * R1);
    orc_generate_randomness(R1, r1);
    size_t qo = 0, ro = 0;
    oF *q1 = qpoly, *rr1 = r_out;
    orc_prove_linear_code(aggr_c, rows2, trs, r1, q1, rr1, vr, fin);
    qo += 3 * R1; ro += R1;
    oF *b1 = (oF *)malloc(sizeof(oF) * rows2);
    orc_precompute_beta(rr1, R1, b1);
    oF *evals = (oF *)malloc(sizeof(oF) * cols);
    for (size_t i = 0; i < cols; i++) {
        oF a = fint(0);
        for (size_t j = 0; j < (size_t)trs; j++) a = f_add(a, f_mul(b1[j], Mp[j * cols + i]));
        for (size_t j = 0; j < (size_t)trs; j++) a = f_add(a, f_mul(b1[j + trs], C[j * cols + i]));
        evals[i] = a;
    }
    oF p17 = fint(021);   /* F(021) in the reference is an OCTAL literal = 17 (src/PC_utils.cpp:322) */
    oF *q2 = qpoly + qo, *rr2 = r_out + ro;
    orc_sumcheck2(sv, evals, cols, &p17, q2, rr2, vr + 2, fin + 1);
    qo += 3 * logc; ro += logc;
    oF c2 = f_add(f_add(q2[0], q2[1]), f_add(q2[2], q2[2]));            /* q(0)+q(1) = a + b + 2c */
    checks[0] = (c2.re == vr[1].re && c2.im == vr[1].im);                /* == P1.vr[1] ("Error recursion 1") */
    size_t big = rows2 * cols;
    oF *buff1 = (oF *)malloc(sizeof(oF) * big), *buff2 = (oF *)calloc(big, sizeof(oF));
    memcpy(buff1, Mp, sizeof(oF) * (size_t)trs * cols); memcpy(buff1 + (size_t)trs * cols, C, sizeof(oF) * (size_t)trs * cols);
    oF s2 = fint((uint64_t)random()); scalars_out[2] = s2;
    oF pw = s2;
    for (int q = 0; q < queries; q++) { buff2[Iv[q]] = pw; pw = f_mul(pw, s2); }
    oF p121 = fint(121);
    int R3 = R1 + logc;
    oF *q3 = qpoly + qo, *rr3 = r_out + ro;
    orc_sumcheck2(buff1, buff2, big, &p121, q3, rr3, vr + 4, fin + 2);
    qo += 3 * R3; ro += R3;
    oF a = fint((uint64_t)random()); scalars_out[3] = a;
    oF *rcat = (oF *)malloc(sizeof(oF) * R3);
    memcpy(rcat, rr2, sizeof(oF) * logc); memcpy(rcat + logc, rr1, sizeof(oF) * R1);
    oF *bb = (oF *)malloc(sizeof(oF) * big);
    orc_precompute_beta(rcat, R3, buff2);            /* buff2 <- beta(r) */
    orc_precompute_beta(rr3, R3, bb);
    for (size_t i = 0; i < big; i++) buff2[i] = f_add(buff2[i], f_mul(a, bb[i]));
    oF p312 = fint(312);
    oF *q4 = qpoly + qo, *rr4 = r_out + ro;
    orc_sumcheck2(buff2, buff1, big, &p312, q4, rr4, vr + 6, fin + 3);
    qo += 3 * R3; ro += R3;
    oF c4 = f_add(f_add(q4[0], q4[1]), f_add(q4[2], q4[2]));
    oF want4 = f_add(f_mul(a, vr[4]), vr[3]);                            /* a*P3.vr[0] + P2.vr[1] ("Error recursion 2") */
    checks[1] = (c4.re == want4.re && c4.im == want4.im);
    /* y1 = evaluate_vector(M', r), r = P4.randomness minus its last entry; P5 = prove_fft_matrix */
    oF y1; orc_evaluate_vector(Mp, (size_t)trs * cols, rr4, R3 - 1, &y1); scalars_out[4] = y1;
    oF *q5 = qpoly + qo, *rr5 = r_out + ro;
    orc_prove_fft_matrix(aggr, trs, cols / 2, rr4, q5, rr5, vr + 8, fin + 4);
    oF c5 = f_add(f_add(q5[0], q5[1]), f_add(q5[2], q5[2]));
    checks[2] = (c5.re == y1.re && c5.im == y1.im);                      /* prove_fft_matrix's own check */
    free(beta); free(aggr); free(T); free(Mp); free(Iv); free(sv); free(aggr_c); free(r1); free(b1); free(evals); free(buff1); free(buff2); free(rcat); free(bb);
    return (int)(qo / 3 + logc);
}

/* ------------------------------------------------------------------------------------------ */
/* Elastic_PC streaming commit: src/Elastic_PC.cpp:174-285; stream src/witness_stream.cpp:2405-11 */
/* ------------------------------------------------------------------------------------------ */
void orc_read_stream_pc(size_t B, oF *out) {
    oF n = fint(322322);
    for (size_t i = 0; i < B; i++) { out[i] = n; n = f_add(f_mul(n, n), fint((uint64_t)i)); }
}
/* _compute_tensorcode (src/PC_utils.cpp:9-64) equals compute_tensorcode on the same globals. */
size_t orc_elastic_commit(size_t N, size_t B, int opt, uint8_t *levels_out) {
    int lin, trs;
    if (opt == 1) { lin = 0; trs = (int)(B >> 11); } else { lin = 1; trs = (int)(B >> 14); orc_expander_init_store(trs); }
    size_t cols = 2 * B / (size_t)trs, rows = 2 * (size_t)trs, T = rows * cols; /* T = 4B */
    oF *buff = (oF *)malloc(sizeof(oF) * B), *tensor = (oF *)malloc(sizeof(oF) * T);
    oF *ci[3]; for (int i = 0; i < 3; i++) ci[i] = (oF *)malloc(sizeof(oF) * T);
    memset(levels_out, 0, 32 * T);
    size_t chunks = N / B;
    for (size_t i = 0; i < chunks; i++) {
        orc_read_stream_pc(B, buff);
        int nz = 0;
        for (size_t j = 0; j < B; j++) if (!fis0(buff[j])) { nz = 1; break; }
        if (nz) orc_compute_tensorcode(buff, B, trs, lin, tensor); else memset(tensor, 0, sizeof(oF) * T);
        if (i % 4 != 3) memcpy(ci[i % 4], tensor, sizeof(oF) * T);
        else for (size_t p = 0; p < T; p++) {
            /* Elastic_PC.cpp:238-239 passes (ci0[counter], ci1[counter], ci2[counter++], tensor[j][k])
             * as arguments of ONE call: the evaluation order is unspecified in C++, and the
             * reference as built by GCC (x86-64, right-to-left) reads ci0/ci1 at counter+1.  We
             * restate the as-built behaviour (checked against oracle/_ref).  For the very last
             * position the reference reads one element past the end of two heap arrays; those
             * arrays are >= 1 MiB (mmap'd, zero page tail) so it reads zeros -- we use zeros.
             * Only leaf T-1 (odd index, never hashed into a parent: left|left quirk) depends on it. */
            oF z = fint(0);
            oF x[4] = {p + 1 < T ? ci[0][p + 1] : z, p + 1 < T ? ci[1][p + 1] : z, ci[2][p], tensor[p]};
            hash_md(x, levels_out + 32 * p, levels_out + 32 * p);
        }
    }
    free(buff); free(tensor); for (int i = 0; i < 3; i++) free(ci[i]);
    return create_tree(levels_out, T);
}


/* ------------------------------------------------------------------------------------------ */
/* Elastic_PC open, RS x RS (test_Elastic_PC option 1): src/Elastic_PC.cpp:625-726 with         */
/* aggregate (:316-347), compute_aggregation_reply + update_reply (:487-533, 59-111) and          */
/* recursive_prover_RS (src/PC_utils.cpp:396-512) up to its closing shockwave_prove(C_f, r_x),     */
/* which the caller composes (orc_shockwave_prove_ex) with the libc generator running on.         */
/* Passes 2 and 3 read the stream through read_stream, whose default branch serves the "test"     */
/* descriptor: v[i] = F(i % 1024 + 1) (src/witness_stream.cpp:2348-2352), every chunk alike.       */
/* Option 2 (RS x expander) is NOT restated: update_reply_spielman (:431-485) indexes a            */
/* tensor_row_size-long copy of the un-encoded column with rows >= tensor_row_size (:465-478),     */
/* a read past the vector -- there is no defined result to be bit-exact with.                      */
/* ------------------------------------------------------------------------------------------ */
void orc_read_stream(size_t B, oF *out) { for (size_t i = 0; i < B; i++) out[i] = fint((uint64_t)(i % 1024) + 1); }
/* Stream model for the streaming provers.  kind 0: the reference's default branch (every read alike).  kind 1 (tests only, no
 * counterpart in the reference): read number c since the last reset returns splitmix_field(n, seed + c) -- full-range values that
 * differ from read to read, so that chunk-order mistakes cannot hide behind a repeating stream. */
static int g_stream_kind = 0; static uint64_t g_stream_seed = 0, g_stream_count = 0;
void orc_stream_config(int kind, uint64_t seed) { g_stream_kind = kind; g_stream_seed = seed; g_stream_count = 0; }
static void stream_reset(void) { g_stream_count = 0; }
static void stream_read(oF *dst, size_t n) {
    if (g_stream_kind == 0) { orc_read_stream(n, dst); return; }
    const uint64_t sd = g_stream_seed + g_stream_count++;
    for (size_t i = 0; i < 2 * n; i++) {
        uint64_t z = sd * 0x632BE59BD9B4E019ULL + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; z ^= z >> 31;
        if (i & 1) dst[i / 2].im = z % P61; else dst[i / 2].re = z % P61;
    }
}

void orc_elastic_aggregate(size_t N, size_t B, const oF *beta, oF *aggr_out, uint8_t *cf_root) {
    oF *buff = (oF *)malloc(sizeof(oF) * B);
    memset(aggr_out, 0, sizeof(oF) * B);
    stream_reset();
    for (size_t i = 0; i < N / B; i++) {                 /* :327-334 */
        stream_read(buff, B);
        for (size_t j = 0; j < B; j++) aggr_out[j] = f_add(aggr_out[j], f_mul(beta[i], buff[j]));
    }
    if (cf_root) {                                       /* C_f = shockwave_commit(buff = aggr, 32) (:343-346) */
        oF *enc = (oF *)malloc(sizeof(oF) * 2 * B); uint8_t *lv = (uint8_t *)malloc(64 * (2 * B / 32) * 2);
        size_t cnt = orc_shockwave_commit(aggr_out, B, 32, enc, lv); memcpy(cf_root, lv + 32 * (cnt - 1), 32);
        free(enc); free(lv);
    }
    free(buff);
}
/* update_reply (:59-111, !linear_time): rows FFT'd to twice their length, then per query the queried column (tensor_row_size entries,
 * zero-padded to twice that) is transformed and its queried row appended.  A chunk that is all zero is skipped (:510-517): nothing is
 * appended for it.  reply: nq x (N/B) row-major; returns the number of entries appended per query. */
size_t orc_elastic_reply(size_t N, size_t B, const uint64_t *Iq, size_t nq, oF *reply) {
    const size_t trs = B >> 11, half = B / trs, cols = 2 * half, K = N / B;
    const int logc = (int)log2((double)cols), logr = (int)log2((double)(2 * trs));
    oF *buff = (oF *)malloc(sizeof(oF) * B), *T = (oF *)malloc(sizeof(oF) * trs * cols), *col = (oF *)malloc(sizeof(oF) * 2 * trs);
    size_t filled = 0;
    stream_reset();
    for (size_t i = 0; i < K; i++) {
        stream_read(buff, B);
        int nz = 0;
        for (size_t j = 0; j < B; j++) if (!fis0(buff[j])) { nz = 1; break; }
        if (!nz) continue;
        memset(T, 0, sizeof(oF) * trs * cols);
        for (size_t r = 0; r < trs; r++) { memcpy(T + r * cols, buff + r * half, sizeof(oF) * half); orc_fft_cached(T + r * cols, logc, 0); }
        for (size_t q = 0; q < nq; q++) {
            memset(col, 0, sizeof(oF) * 2 * trs);
            for (size_t r = 0; r < trs; r++) col[r] = T[r * cols + Iq[2 * q]];
            orc_fft(col, logr, 0);
            reply[q * K + filled] = col[Iq[2 * q + 1]];
        }
        filled++;
    }
    free(buff); free(T); free(col);
    return filled;
}
static int cmp_sz(const void *a, const void *b) { size_t x = *(const size_t *)a, y = *(const size_t *)b; return x < y ? -1 : x > y; }
static size_t next_pow2(size_t l) { size_t p = 1; while (p < l) p <<= 1; return p; }
/* recursive_prover_RS (src/PC_utils.cpp:396-512) on an aggregated vector of B elements seen as trs rows (globals tensor_row_size, C_f), for the
 * queries Iq = (column, row) pairs.  qpoly / r_out / vr / fin hold P0, P2, P3, P5 back to back (rounds R0 = log2(np2 * 2trs), log2(2trs),
 * log2(2B), log2(2B/trs)); rx = P5.randomness[0], the point shockwave_prove(C_f, .) is then run on by the caller.
 * checks[0]: P2's claimed sum == P0.vr[0]; checks[1]: P5's == P3.vr[0] (prove_fft_matrix's own exit(-1) tests, src/sumcheck.cpp:3016-3019). */
static int rs_prover(const oF *aggr, size_t B, size_t trs, const uint64_t *Iq, int queries, int *ncols_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, oF *rx_out) {
    const size_t half = B / trs, cols = 2 * half, rows2 = 2 * trs;
    const int logc = (int)log2((double)cols), logr = (int)log2((double)rows2), logt = (int)log2((double)trs);
    size_t *cs = (size_t *)malloc(sizeof(size_t) * (size_t)queries);
    for (int q = 0; q < queries; q++) cs[q] = Iq[2 * q];
    qsort(cs, (size_t)queries, sizeof(size_t), cmp_sz);                       /* I_sorted's first entries / I_t (:128-142) */
    size_t *col = (size_t *)malloc(sizeof(size_t) * (size_t)queries), nc = 0;
    for (int q = 0; q < queries; q++) if (q == 0 || cs[q] != cs[q - 1]) col[nc++] = cs[q];
    const size_t np2 = next_pow2(nc);
    if (ncols_out) *ncols_out = (int)nc;
    oF *out1 = (oF *)calloc(trs * cols, sizeof(oF));                          /* rows of the aggregate, RS-encoded (:406-420) */
    for (size_t i = 0; i < trs; i++) { memcpy(out1 + i * cols, aggr + i * half, sizeof(oF) * half); orc_fft_cached(out1 + i * cols, logc, 0); }
    oF *sel = (oF *)calloc(np2 * trs, sizeof(oF)), *out3 = (oF *)calloc(np2 * rows2, sizeof(oF));
    for (size_t i = 0; i < nc; i++) {                                         /* selected columns and their codewords (:422-452) */
        for (size_t j = 0; j < trs; j++) { sel[i * trs + j] = out1[j * cols + col[i]]; out3[i * rows2 + j] = sel[i * trs + j]; }
        orc_fft_cached(out3 + i * rows2, logr, 0);
    }
    oF *bt = (oF *)calloc(np2 * rows2, sizeof(oF));
    oF *rq = (oF *)malloc(sizeof(oF) * (size_t)queries);
    orc_generate_randomness(queries, rq);                                     /* (:459) */
    {   size_t counter = 0;                                                   /* (:461-470): the sorted column walk indexes the UNSORTED rows */
        for (int i = 0; i < queries; i++) {
            if (col[counter] != cs[i]) counter++;
            const size_t at = counter * rows2 + Iq[2 * i + 1];
            bt[at] = f_add(bt[at], rq[i]);
        } }
    const int R0 = (int)log2((double)(np2 * rows2));
    oF p323 = fint(323);
    size_t qo = 0, ro = 0;
    oF *q0 = qpoly, *r0 = r_out;
    orc_sumcheck2(out3, bt, np2 * rows2, &p323, q0, r0, vr, fin);             /* P0 (:474) */
    qo += 3 * (size_t)R0; ro += (size_t)R0;
    oF *q2 = qpoly + qo, *r2 = r_out + ro;
    orc_prove_fft_matrix(sel, np2, trs, r0, q2, r2, vr + 2, fin + 1);        /* P2 (:480) */
    { oF c = f_add(f_add(q2[0], q2[1]), f_add(q2[2], q2[2])); checks[0] = (c.re == vr[0].re && c.im == vr[0].im); }
    qo += 3 * (size_t)logr; ro += (size_t)logr;
    /* P2.randomness[0] = sumcheck challenges (logr) | r1 = P0.r[logr ..]; r_point = entries from index log2(trs) on (:482-485) */
    const int np = 1 + (R0 - logr);
    oF *rpt = (oF *)malloc(sizeof(oF) * (size_t)np);
    rpt[0] = r2[logt];
    for (int i = 0; i < R0 - logr; i++) rpt[1 + i] = r0[logr + i];
    oF *rb = (oF *)malloc(sizeof(oF) * ((size_t)1 << np));
    orc_precompute_beta(rpt, np, rb);
    oF *b2 = (oF *)calloc(trs * cols, sizeof(oF));                            /* (:489-496) */
    for (size_t i = 0; i < nc; i++) for (size_t j = 0; j < trs; j++) b2[col[i] + j * cols] = rb[i];
    oF *q3 = qpoly + qo, *r3 = r_out + ro;
    orc_sumcheck2(out1, b2, trs * cols, &p323, q3, r3, vr + 4, fin + 2);      /* P3 (:498) */
    qo += 3 * (size_t)(logt + logc); ro += (size_t)(logt + logc);
    oF *q5 = qpoly + qo, *r5 = r_out + ro;
    orc_prove_fft_matrix(aggr, trs, half, r3, q5, r5, vr + 6, fin + 3);      /* P5 (:503) */
    { oF c = f_add(f_add(q5[0], q5[1]), f_add(q5[2], q5[2])); checks[1] = (c.re == vr[4].re && c.im == vr[4].im); }
    /* r_x = P5.randomness[0] = its sumcheck challenges (logc) followed by r1 = P3.r[logc .. logc + log2 trs) (src/sumcheck.cpp:3021-3023) */
    memcpy(rx_out, r5, sizeof(oF) * (size_t)logc);
    memcpy(rx_out + logc, r3 + logc, sizeof(oF) * (size_t)logt);
    free(cs); free(col); free(out1); free(sel); free(out3); free(bt); free(rq); free(rpt); free(rb); free(b2);
    return R0 + logr + (logt + logc) + logc;
}
/* Elastic_PC::open option 1 up to (not including) shockwave_prove; transcript layout as rs_prover.
 * commit_levels: the commitment tree (4B leaves) or NULL; paths: queries x log2(4B) hashes. */
int orc_elastic_open_rs(size_t N, size_t B, const oF *x, int queries, const uint8_t *commit_levels, uint32_t *I_out, oF *rv0_out, oF *aggr_out, uint8_t *cf_root,
                        oF *reply_out, uint8_t *paths_out, int *ncols_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, oF *rx_out) {
    const size_t trs = B >> 11, half = B / trs, cols = 2 * half, rows2 = 2 * trs, K = N / B;
    const int logK = (int)log2((double)K);
    /* open (:625-655): beta over the chunk variables, r_v[0], the queries */
    oF *beta = (oF *)malloc(sizeof(oF) * K);
    orc_precompute_beta(x, logK, beta);
    orc_generate_randomness(1, rv0_out);
    uint64_t *Iq = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (size_t)queries);
    for (int q = 0; q < queries; q++) {
        Iq[2 * q] = (uint64_t)(rand() % (long)cols); Iq[2 * q + 1] = (uint64_t)(rand() % (long)rows2);
        I_out[2 * q] = (uint32_t)Iq[2 * q]; I_out[2 * q + 1] = (uint32_t)Iq[2 * q + 1];
    }
    orc_elastic_aggregate(N, B, beta, aggr_out, cf_root);
    if (reply_out) orc_elastic_reply(N, B, Iq, (size_t)queries, reply_out);
    if (commit_levels && paths_out) {                     /* open_tree_blake(Commitment_MT, I[i], 2B/trs) (:684-687) */
        const int depth = (int)log2((double)(4 * B));
        for (int q = 0; q < queries; q++) orc_open_tree_blake(commit_levels, 4 * B, Iq[2 * q], Iq[2 * q + 1], cols, paths_out + (size_t)q * depth * 32);
    }
    const int rounds = rs_prover(aggr_out, B, trs, Iq, queries, ncols_out, qpoly, r_out, vr, fin, checks, rx_out);
    free(beta); free(Iq);
    return rounds;
}
/* ------------------------------------------------------------------------------------------ */
/* Elastic_PC open, RS x expander (test_Elastic_PC option 2, linear_time == true):              */
/* aggregate()'s linear_time branch (src/Elastic_PC.cpp:348-413), compute_aggregation_reply ->    */
/* update_reply_spielman (:431-485, 487-533) and recursive_prover_Spielman_stream                 */
/* (src/PC_utils.cpp:168-270) up to its two shockwave_prove calls, which the caller composes.     */
/* aggregate / compute_aggregation_reply are pinned by oracle/_ref (tests/golden/elastic_open2.npz) */
/* AS BUILT: update_reply_spielman's `buff2 = buff` for a column with a queried parity row shrinks  */
/* the 2*trs-long vector to trs entries and the reply loop then reads buff2[row >= trs] past      */
/* size() but inside the retained storage (libstdc++ copy-assignment keeps it; F's destructor is   */
/* trivial) -- i.e. the parity of the LAST column that went through encode_monolithic in this      */
/* chunk, or zero before any did.  oracle/check_elastic_open2_determinism.py shows the real         */
/* reference returns the same bytes from fresh processes with different heap histories.           */
/* Restated behind `stale_parity_quirk` (1 = as built; 0 = every column encoded, what the author   */
/* presumably meant, kept only to show the tests can tell the two apart).                          */
/* ------------------------------------------------------------------------------------------ */
/* encode_monolithic writes only the n + L + R codeword entries of dst (src/linear_code_encode.h:114-118); the tail of a 2n buffer keeps its contents */
static long long encode_into(const oF *src, oF *dst, long long n) {
    oF *tmp = (oF *)calloc((size_t)(2 * n) + 16, sizeof(oF));
    long long len = encode_rec(src, tmp, n, 0);
    memcpy(dst, tmp, sizeof(oF) * (size_t)len);
    free(tmp);
    return len;
}
/* columns = sorted distinct queried columns; a column is "remaining" when one of its queried rows is a parity row (:365-381).
 * Returns nc; ucol[nc], flag[nc] (1 = remaining), and per query its index into ucol. */
static size_t open2_columns(const uint64_t *Iq, size_t nq, size_t trs, size_t *ucol, uint8_t *flag, size_t *qidx) {
    size_t *cs = (size_t *)malloc(sizeof(size_t) * nq), nc = 0;
    for (size_t q = 0; q < nq; q++) cs[q] = Iq[2 * q];
    qsort(cs, nq, sizeof(size_t), cmp_sz);
    for (size_t q = 0; q < nq; q++) if (q == 0 || cs[q] != cs[q - 1]) ucol[nc++] = cs[q];
    memset(flag, 0, nc);
    for (size_t q = 0; q < nq; q++) {
        size_t lo = 0, hi = nc;
        while (lo + 1 < hi) { size_t mid = (lo + hi) / 2; if (ucol[mid] <= Iq[2 * q]) lo = mid; else hi = mid; }
        qidx[q] = lo;
        if (Iq[2 * q + 1] >= trs) flag[lo] = 1;
    }
    free(cs);
    return nc;
}
/* aggregate(), linear_time branch.  aux_out: nr x 2trs (aux_commit); rem_out: the nr remaining columns; tensor_out (nullable):
 * aggregated_tensor, trs x 2B/trs.  Returns nr. */
size_t orc_elastic_aggregate2(size_t N, size_t B, const oF *beta, const uint64_t *Iq, size_t nq, oF *aggr_out, uint8_t *cf_root, uint8_t *cc_root,
                              oF *aux_out, oF *tensor_out) {
    const size_t trs = B >> 14, half = B / trs, cols = 2 * half, rows2 = 2 * trs;
    const int logc = (int)log2((double)cols);
    orc_elastic_aggregate(N, B, beta, aggr_out, cf_root);                     /* :327-334, C_f = shockwave_commit(aggregated_vector, 32) (:349) */
    size_t *ucol = (size_t *)malloc(sizeof(size_t) * nq), *qidx = (size_t *)malloc(sizeof(size_t) * nq); uint8_t *flag = (uint8_t *)malloc(nq);
    const size_t nc = open2_columns(Iq, nq, trs, ucol, flag, qidx);
    oF *T = (oF *)calloc(trs * cols, sizeof(oF)), *col = (oF *)malloc(sizeof(oF) * trs);
    for (size_t i = 0; i < trs; i++) { memcpy(T + i * cols, aggr_out + i * half, sizeof(oF) * half); orc_fft_cached(T + i * cols, logc, 0); }   /* :365-375 */
    if (tensor_out) memcpy(tensor_out, T, sizeof(oF) * trs * cols);
    size_t nr = 0;
    for (size_t i = 0; i < nc; i++) if (flag[i]) {                            /* aux_commit[i] = encode_monolithic(column) (:394-403) */
        for (size_t j = 0; j < trs; j++) col[j] = T[j * cols + ucol[i]];
        memset(aux_out + nr * rows2, 0, sizeof(oF) * rows2);
        encode_into(col, aux_out + nr * rows2, (long long)trs);
        nr++;
    }
    if (cc_root) {                                                            /* C_c = shockwave_commit(pad(convert2vector(aux_commit)), 32) (:407-411) */
        const size_t np = next_pow2(nr * rows2);
        oF *flat = (oF *)calloc(np, sizeof(oF)); memcpy(flat, aux_out, sizeof(oF) * nr * rows2);
        oF *enc = (oF *)malloc(sizeof(oF) * 2 * np); uint8_t *lv = (uint8_t *)malloc(64 * (2 * np / 32) * 2);
        size_t cnt = orc_shockwave_commit(flat, np, 32, enc, lv); memcpy(cc_root, lv + 32 * (cnt - 1), 32);
        free(flat); free(enc); free(lv);
    }
    free(ucol); free(qidx); free(flag); free(T); free(col);
    return nr;
}
/* compute_aggregation_reply under linear_time: per non-zero chunk update_reply_spielman (:431-485).  reply: nq x (N/B) row-major, the entries
 * in the order the reference appends them: sorted distinct column by column, within a column in query order (column_map).  reply_q[k] says
 * which reply row k belongs to which query... the reference's reply[counter++] rows are NOT in query order: row `counter` belongs to the
 * counter-th (column-sorted, stable) query -- kept.  Returns the entries appended per row. */
size_t orc_elastic_reply2(size_t N, size_t B, const uint64_t *Iq, size_t nq, oF *reply, int stale_parity_quirk) {
    const size_t trs = B >> 14, half = B / trs, cols = 2 * half, rows2 = 2 * trs, K = N / B;
    const int logc = (int)log2((double)cols);
    size_t *ucol = (size_t *)malloc(sizeof(size_t) * nq), *qidx = (size_t *)malloc(sizeof(size_t) * nq); uint8_t *flag = (uint8_t *)malloc(nq);
    const size_t nc = open2_columns(Iq, nq, trs, ucol, flag, qidx);
    /* column_map[c] = rows of the queries on column c in query order: bucket the queries by column index, stably */
    size_t *start = (size_t *)calloc(nc + 1, sizeof(size_t)), *ord = (size_t *)malloc(sizeof(size_t) * nq);
    for (size_t q = 0; q < nq; q++) start[qidx[q] + 1]++;
    for (size_t i = 0; i < nc; i++) start[i + 1] += start[i];
    {   size_t *fill = (size_t *)malloc(sizeof(size_t) * nc); memcpy(fill, start, sizeof(size_t) * nc);
        for (size_t q = 0; q < nq; q++) ord[fill[qidx[q]]++] = q;
        free(fill); }
    oF *buff = (oF *)malloc(sizeof(oF) * B), *T = (oF *)malloc(sizeof(oF) * trs * cols), *col = (oF *)malloc(sizeof(oF) * trs), *buff2 = (oF *)malloc(sizeof(oF) * rows2);
    size_t filled = 0;
    stream_reset();
    for (size_t i = 0; i < K; i++) {
        stream_read(buff, B);
        int nz = 0;
        for (size_t j = 0; j < B; j++) if (!fis0(buff[j])) { nz = 1; break; }
        if (!nz) continue;                                                    /* :510-517 */
        memset(T, 0, sizeof(oF) * trs * cols);
        for (size_t r = 0; r < trs; r++) { memcpy(T + r * cols, buff + r * half, sizeof(oF) * half); orc_fft_cached(T + r * cols, logc, 0); }   /* :445-453 */
        memset(buff2, 0, sizeof(oF) * rows2);                                 /* vector<F> buff2(2*tensor_row_size) (:455) */
        size_t counter = 0;
        for (size_t c = 0; c < nc; c++) {
            for (size_t j = 0; j < trs; j++) col[j] = T[j * cols + ucol[c]];
            if (flag[c] && stale_parity_quirk) memcpy(buff2, col, sizeof(oF) * trs);   /* buff2 = buff: the first trs entries only; the rest is stale (:470-472) */
            else encode_into(col, buff2, (long long)trs);                     /* (:473) */
            for (size_t k = start[c]; k < start[c + 1]; k++) reply[(counter++) * K + filled] = buff2[Iq[2 * ord[k] + 1]];   /* :476-478 */
        }
        filled++;
    }
    free(ucol); free(qidx); free(flag); free(start); free(ord); free(buff); free(T); free(col); free(buff2);
    return filled;
}
/* src/sumcheck.cpp:2989-3027 prove_fft_matrix with the transcript seed given: the reference seeds with r[r.size()-1], and
 * recursive_prover_Spielman_stream hands it an r that is one entry longer than the variables it uses */
static void prove_fft_matrix_prev(const oF *M, size_t rows, size_t cols, const oF *rr, const oF *prev, oF *qpoly, oF *r, oF *vr, oF *fin) {
    size_t C2 = 2 * cols; int k2 = (int)log2((double)C2), k1 = (int)log2((double)rows);
    oF *Mt = (oF *)calloc(C2 * rows, sizeof(oF)), *arr = (oF *)malloc(sizeof(oF) * C2), *Fg = (oF *)malloc(sizeof(oF) * C2);
    for (size_t i = 0; i < rows; i++) for (size_t c = 0; c < cols; c++) Mt[c * rows + i] = M[i * cols + c];
    orc_prepare_matrix(Mt, C2, rows, rr + k2, k1, arr);
    oF one = fint(1);
    orc_phi_g_init(rr, k2, &one, 0, Fg);
    orc_sumcheck2(Fg, arr, C2, prev, qpoly, r, vr, fin);
    free(Mt); free(arr); free(Fg);
}
/* Elastic_PC::open option 2 up to (not including) the two shockwave_prove calls.  Transcripts P1 (log2 2trs rounds), P2 (log2 cols), P3
 * (log2 np, np = nr*2trs rounded up to a power of two), P5 (log2 cols) back to back; vr 4 x 2, fin 4; scal = s[0], s2, y1;
 * checks[0] = prove_fft_matrix's exit(-1) sum check (src/sumcheck.cpp:3016-3019); rx = P5.randomness[0] minus its last entry (log2 B F).
 * aux_out: nq x 2trs capacity (nr rows used).  reply rows are in the reference's order (orc_elastic_reply2).  Returns the total rounds. */
int orc_elastic_open_spielman(size_t N, size_t B, const oF *x, int queries, const uint8_t *commit_levels, int stale_parity_quirk, uint32_t *I_out, oF *rv0_out,
                              oF *aggr_out, uint8_t *roots /* C_f, C_c */, oF *reply_out, uint8_t *paths_out, int *nr_out, oF *aux_out, oF *scal, oF *qpoly, oF *r_out,
                              oF *vr, oF *fin, int *checks, oF *rx_out) {
    const size_t trs = B >> 14, half = B / trs, cols = 2 * half, rows2 = 2 * trs, K = N / B, nq = (size_t)queries;
    const int logK = (int)log2((double)K), logc = (int)log2((double)cols), R1 = (int)log2((double)rows2), logt = R1 - 1;
    oF *beta = (oF *)malloc(sizeof(oF) * K);
    orc_precompute_beta(x, logK, beta);
    orc_generate_randomness(1, rv0_out);                                      /* r_v[0] (:645) */
    uint64_t *Iq = (uint64_t *)malloc(sizeof(uint64_t) * 2 * nq);
    for (size_t q = 0; q < nq; q++) {                                         /* (:650-655) */
        Iq[2 * q] = (uint64_t)(rand() % (long)cols); Iq[2 * q + 1] = (uint64_t)(rand() % (long)rows2);
        I_out[2 * q] = (uint32_t)Iq[2 * q]; I_out[2 * q + 1] = (uint32_t)Iq[2 * q + 1];
    }
    oF *M = (oF *)malloc(sizeof(oF) * trs * cols);
    const size_t nr = orc_elastic_aggregate2(N, B, beta, Iq, nq, aggr_out, roots, roots + 32, aux_out, M);
    *nr_out = (int)nr;
    if (reply_out) orc_elastic_reply2(N, B, Iq, nq, reply_out, stale_parity_quirk);
    if (commit_levels && paths_out) {                                         /* open_tree_blake(Commitment_MT, I[i], 2B/trs) (:684-687) */
        const int depth = (int)log2((double)(4 * B));
        for (size_t q = 0; q < nq; q++) orc_open_tree_blake(commit_levels, 4 * B, Iq[2 * q], Iq[2 * q + 1], cols, paths_out + q * (size_t)depth * 32);
    }
    /* recursive_prover_Spielman_stream(aggr_vector, aggr_tensor = M, aux_commit = codewords, I) */
    size_t *ucol = (size_t *)malloc(sizeof(size_t) * nq), *qidx = (size_t *)malloc(sizeof(size_t) * nq); uint8_t *flag = (uint8_t *)malloc(nq);
    const size_t nc = open2_columns(Iq, nq, trs, ucol, flag, qidx);
    oF *s = (oF *)malloc(sizeof(oF) * (nr ? nr : 1));
    s[0] = fint((uint64_t)random()); scal[0] = s[0];                          /* (:209-213) */
    for (size_t i = 1; i < nr; i++) s[i] = f_mul(s[i - 1], s[0]);
    oF *aggr_c = (oF *)calloc(rows2, sizeof(oF));
    for (size_t i = 0; i < nr; i++) for (size_t j = 0; j < rows2; j++) aggr_c[j] = f_add(aggr_c[j], f_mul(s[i], aux_out[i * rows2 + j]));   /* (:214-219) */
    oF *r1 = (oF *)malloc(sizeof(oF) * (size_t)R1);
    orc_generate_randomness(R1, r1);
    size_t qo = 0, ro = 0;
    oF *q1 = qpoly, *rr1 = r_out;
    orc_prove_linear_code(aggr_c, rows2, (long long)trs, r1, q1, rr1, vr, fin);    /* P1 (:221) */
    qo += 3 * (size_t)R1; ro += (size_t)R1;
    oF *b1 = (oF *)malloc(sizeof(oF) * rows2);
    orc_precompute_beta(rr1, R1, b1);
    oF *evals = (oF *)malloc(sizeof(oF) * cols), *sM = (oF *)calloc(cols, sizeof(oF));
    for (size_t i = 0; i < cols; i++) { oF a = fint(0); for (size_t j = 0; j < trs; j++) a = f_add(a, f_mul(b1[j], M[j * cols + i])); evals[i] = a; }   /* (:226-230) */
    { size_t counter = 0; for (size_t i = 0; i < nc; i++) if (flag[i]) sM[ucol[i]] = s[counter++]; }                                                      /* (:231-234) */
    oF p17 = fint(021);
    oF *q2 = qpoly + qo, *rr2 = r_out + ro;
    orc_sumcheck2(sM, evals, cols, &p17, q2, rr2, vr + 2, fin + 1);           /* P2 (:237) */
    qo += 3 * (size_t)logc; ro += (size_t)logc;
    const size_t np = next_pow2(nr * rows2);
    const int R3 = (int)log2((double)np);
    oF *buff1 = (oF *)calloc(np, sizeof(oF)), *buff2 = (oF *)calloc(np, sizeof(oF));
    memcpy(buff1, aux_out, sizeof(oF) * nr * rows2);
    oF s2 = fint((uint64_t)random()); scal[1] = s2;
    if (nq > np) { fprintf(stderr, "orc_elastic_open_spielman: the reference writes %zu query powers into a %zu-entry vector here\n", nq, np); abort(); }
    for (size_t i = 0; i < nq; i++) { buff2[i] = s2; s2 = f_mul(s2, s2); }    /* buff2[i] = s2; s2 = s2*s2 (:243-246): repeated squares at positions 0..nq-1 */
    oF p121 = fint(121);
    oF *q3 = qpoly + qo, *rr3 = r_out + ro;
    orc_sumcheck2(buff1, buff2, np, &p121, q3, rr3, vr + 4, fin + 2);         /* P3 (:248) */
    qo += 3 * (size_t)R3; ro += (size_t)R3;
    /* r = P1.randomness[0] (all R1 entries: the pop_back at :256 comes after the copy) | P2.randomness[0]; y1 = evaluate_vector(M, r) uses its
     * first log2(trs*cols) entries, prove_fft_matrix the same ones, and seeds its transcript with the last one (:255-269) */
    const int nr_r = R1 + logc;
    oF *rcat = (oF *)malloc(sizeof(oF) * (size_t)nr_r);
    memcpy(rcat, rr1, sizeof(oF) * (size_t)R1); memcpy(rcat + R1, rr2, sizeof(oF) * (size_t)logc);
    oF y1; orc_evaluate_vector(M, trs * cols, rcat, logt + logc, &y1); scal[2] = y1;
    oF *q5 = qpoly + qo, *rr5 = r_out + ro;
    prove_fft_matrix_prev(aggr_out, trs, half, rcat, &rcat[nr_r - 1], q5, rr5, vr + 6, fin + 3);   /* P5 (:266) */
    { oF c = f_add(f_add(q5[0], q5[1]), f_add(q5[2], q5[2])); checks[0] = (c.re == y1.re && c.im == y1.im); }
    /* P5.randomness[0] = its logc challenges | r1 = rcat[logc .. logc + logt); pop_back (:268) */
    if (logt > 0) { memcpy(rx_out, rr5, sizeof(oF) * (size_t)logc); memcpy(rx_out + logc, rcat + logc, sizeof(oF) * (size_t)(logt - 1)); }
    else memcpy(rx_out, rr5, sizeof(oF) * (size_t)(logc - 1));              /* trs = 1: r1 is empty and pop_back takes the last sumcheck challenge */
    free(beta); free(Iq); free(M); free(ucol); free(qidx); free(flag); free(s); free(aggr_c); free(r1); free(b1); free(evals); free(sM); free(buff1); free(buff2); free(rcat);
    return R1 + logc + R3 + logc;
}
/* Our_PC open_standard with linear_time == false (test_PC option 1, src/Our_PC.cpp:604-692: 790 queries, tensor_row_size = 128) up to (not
 * including) shockwave_prove(C_f, r_x): r_v[0]; _aggregate (:258-276: the aggregate and C_f = shockwave_commit(aggr, 32), no C_c); the queries
 * (rand() % (2B/trs), rand() % (2 trs)); _compute_aggregation_reply (:291-305: reply[q][i] = _tensor[i][row_q][col_q], tensor = K x 2trs x cols
 * or NULL); open_tree_blake paths (commit_levels: the M-leaf tree or NULL); recursive_prover_RS.  Transcript layout as rs_prover. */
int orc_open_standard_rs(const oF *poly, size_t N, int K, int trs_, const oF *x, int queries, const uint8_t *commit_levels, const oF *tensor, uint32_t *I_out, oF *rv0_out,
                         oF *aggr_out, uint8_t *cf_root, oF *reply_out, uint8_t *paths_out, int *ncols_out, oF *qpoly, oF *r_out, oF *vr, oF *fin, int *checks, oF *rx_out) {
    const size_t B = N / (size_t)K, trs = (size_t)trs_, cols = 2 * B / trs, rows2 = 2 * trs;
    const int logK = (int)log2((double)K);
    oF *beta = (oF *)malloc(sizeof(oF) * (size_t)K);
    orc_precompute_beta(x, logK, beta);
    orc_generate_randomness(1, rv0_out);
    for (size_t j = 0; j < B; j++) aggr_out[j] = fint(0);
    for (int i = 0; i < K; i++) for (size_t j = 0; j < B; j++) aggr_out[j] = f_add(aggr_out[j], f_mul(beta[i], poly[(size_t)i * B + j]));
    {   /* C_f = shockwave_commit(buff, 32) (src/Virgo.cpp:435-517): only its root is reported */
        oF *enc = (oF *)malloc(sizeof(oF) * 2 * B); uint8_t *lv = (uint8_t *)malloc(64 * (2 * B / 32) * 2);
        size_t cnt = orc_shockwave_commit(aggr_out, B, 32, enc, lv);
        memcpy(cf_root, lv + 32 * (cnt - 1), 32);
        free(enc); free(lv);
    }
    uint64_t *Iq = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (size_t)queries);
    for (int q = 0; q < queries; q++) {
        Iq[2 * q] = (uint64_t)(rand() % (long)cols); Iq[2 * q + 1] = (uint64_t)(rand() % (long)rows2);
        I_out[2 * q] = (uint32_t)Iq[2 * q]; I_out[2 * q + 1] = (uint32_t)Iq[2 * q + 1];
    }
    if (reply_out && tensor)
        for (int q = 0; q < queries; q++) for (int i = 0; i < K; i++) reply_out[(size_t)q * K + i] = tensor[((size_t)i * rows2 + Iq[2 * q + 1]) * cols + Iq[2 * q]];
    if (commit_levels && paths_out) {
        const int depth = (int)log2((double)B);
        for (int q = 0; q < queries; q++) orc_open_tree_blake(commit_levels, B, Iq[2 * q], Iq[2 * q + 1], cols, paths_out + (size_t)q * depth * 32);
    }
    const int rounds = rs_prover(aggr_out, B, trs, Iq, queries, ncols_out, qpoly, r_out, vr, fin, checks, rx_out);
    free(beta); free(Iq);
    return rounds;
}


/* ------------------------------------------------------------------------------------------ */
/* Streaming (space-efficient) sumcheck drivers of the multiplication-tree prover:              */
/* read_mul_tree_layer / read_mul_tree_data (src/witness_stream.cpp:2413-2510, the branch for     */
/* every stream but "wiring_consistency_check"), generate_claims_opt (src/sumcheck.cpp:1014-1054), */
/* generate_3product_sumcheck_beta_stream_batch_optimized (:1150-1393) and                         */
/* prove_multiplication_tree_stream_shallow (:1746-1915) without commit_layers / open_layers.      */
/* ------------------------------------------------------------------------------------------ */
/* v[0 .. size): products of 2^layer consecutive stream elements; one read of 2*size elements fills size/2^layer entries of each half */
static void read_mul_tree_layer(oF *v, size_t size, int layer) {
    const size_t seg = (size_t)1 << layer;
    oF *tmp = (oF *)malloc(sizeof(oF) * 2 * size);
    for (size_t i = 0; i < size; i++) v[i] = fint(1);
    size_t counter = 0;
    while (counter != size / 2) {
        stream_read(tmp, 2 * size);
        for (size_t i = 0; i < size / seg; i++) {
            for (size_t j = 0; j < seg; j++) v[counter] = f_mul(v[counter], tmp[i * seg + j]);
            for (size_t j = 0; j < seg; j++) v[counter + size / 2] = f_mul(v[counter + size / 2], tmp[i * seg + j + size]);
            counter++;
        }
    }
    free(tmp);
}
/* V[0]: `size` products of 2^layer consecutive elements (lower half from the first half of every read, upper half from its second
 * half); V[i] (i >= 1): products of 2^distance consecutive entries of V[i-1] */
static void read_mul_tree_data(oF **V, const size_t *vlen, int batches, size_t size, int layer, int distance) {
    const size_t seg = (size_t)1 << layer;
    oF *tmp = (oF *)malloc(sizeof(oF) * size);
    size_t counter = 0;
    while (counter != size / 2) {
        stream_read(tmp, size);
        for (size_t i = 0; i < size / (2 * seg); i++) {
            oF a = tmp[i * seg], b = tmp[i * seg + size / 2];
            for (size_t j = 1; j < seg; j++) { a = f_mul(a, tmp[i * seg + j]); b = f_mul(b, tmp[i * seg + j + size / 2]); }
            V[0][counter] = a; V[0][counter + size / 2] = b; counter++;
        }
    }
    const size_t off = (size_t)1 << distance;
    for (int i = 1; i < batches; i++)
        for (size_t j = 0; j < vlen[i]; j++) { oF a = fint(1); for (size_t k = 0; k < off; k++) a = f_mul(a, V[i - 1][off * j + k]); V[i][j] = a; }
    free(tmp);
}
void orc_read_mul_tree_layer(size_t size, int layer, oF *out) { stream_reset(); read_mul_tree_layer(out, size, layer); }
/* V levels back to back in `out` (4B, 4B >> distance, ...) */
void orc_read_mul_tree_data(size_t size, int layer, int distance, int batches, oF *out) {
    oF *V[16]; size_t vlen[16]; size_t o = 0;
    for (int i = 0; i < batches; i++) { V[i] = out + o; vlen[i] = size >> (i * distance); o += vlen[i]; }
    stream_reset(); read_mul_tree_data(V, vlen, batches, size, layer, distance);
}
/* r: batches x rlen (row-major); new_r: batches rows, row i of 1 + (logB - i*distance) + log2(R) entries (stride new_r_ld);
 * transcript: P1 (batch_3product_sumcheck: rounds1 = logB rounds of 4 F), P2 (2-product over R: 3 F per round).
 * checks: [0] every K_partial == old_claims ("Error in sumcheck 0", printed only), [1] P1's claim == Kf, [2] sum b.vr == P2's claim. */
int orc_sumcheck3_stream_batch(size_t fd_size, size_t B, const oF *r, int rlen, int batches, int distance, int layer_id, const oF *old_claims, int n_old,
                               oF *new_claims, oF *new_r, int new_r_ld, oF *cpoly1, oF *r1, oF *vr1, oF *qpoly2, oF *r2, oF *vr2, oF *fin2, oF *R_out, int *checks) {
    const size_t size = fd_size >> layer_id; const int logB = (int)log2((double)B);
    oF *f1[16], *f2[16], *f3[16], *b1[16], *b2[16], *b3[16], *rb[16], *V[16]; size_t sz[16] = {0}, vlen[16] = {0}, rbn[16] = {0};
    for (int i = 0; i < batches; i++) {
        sz[i] = B >> (i * distance); vlen[i] = (4 * B) >> (i * distance);
        f1[i] = (oF *)malloc(sizeof(oF) * sz[i]); f2[i] = (oF *)malloc(sizeof(oF) * sz[i]); f3[i] = (oF *)malloc(sizeof(oF) * sz[i]);
        b1[i] = (oF *)malloc(sizeof(oF) * sz[i]); b2[i] = (oF *)malloc(sizeof(oF) * sz[i]); b3[i] = (oF *)malloc(sizeof(oF) * sz[i]);
        V[i] = (oF *)malloc(sizeof(oF) * vlen[i]);
        const int n_init = logB - i * distance, n_rem = (int)log2((double)(size / 2)) - i * distance - n_init;
        orc_precompute_beta(r + (size_t)i * rlen, n_init, b3[i]); memcpy(f3[i], b3[i], sizeof(oF) * sz[i]);
        rbn[i] = (size_t)1 << n_rem; rb[i] = (oF *)malloc(sizeof(oF) * rbn[i]);
        orc_precompute_beta(r + (size_t)i * rlen + n_init, n_rem, rb[i]);
    }
    const size_t nch = size / (4 * B), half = rbn[0] / 2;
    stream_reset();
    read_mul_tree_data(V, vlen, batches, 4 * B, layer_id, distance);
    oF Kp[16], a[16];
    for (int i = 0; i < batches; i++) {
        Kp[i] = fint(0);
        for (size_t j = 0; j < sz[i]; j++) { f1[i][j] = V[i][2 * j]; f2[i][j] = V[i][2 * j + 1]; }
        for (size_t j = 0; j < sz[i]; j++) Kp[i] = f_add(Kp[i], f_mul(f_mul(f1[i][j], f2[i][j]), f3[i][j]));
    }
    orc_generate_randomness(batches, a);
    oF Kf = fint(0);
    size_t nR = 1; oF *R = (oF *)malloc(sizeof(oF) * (2 * nch + 1)); R[0] = fint(1);
    for (int i = 0; i < batches; i++) { Kf = f_add(Kf, f_mul(a[i], Kp[i])); Kp[i] = f_mul(Kp[i], rb[i][0]); }
    /* one batch_prod step (src/sumcheck.cpp:1093-1136) on the chunk halves currently in b1/b2, remaining_betas index idx */
#define BATCH_PROD_STEP(idx) do {                                                                                               \
        oF K1 = fint(0), K2 = fint(0), K3[16], rnd = R[nR - 1];                                                                 \
        for (int j = 0; j < batches; j++) { oF K[3] = {fint(0), fint(0), fint(0)};                                              \
            orc_batch_prod_terms(b1[j], b2[j], b3[j], f1[j], f2[j], f3[j], sz[j], K);                                           \
            K1 = f_add(K1, f_mul(a[j], K[0])); K2 = f_add(K2, f_mul(a[j], K[1])); K3[j] = K[2]; }                               \
        rnd = mimc_hash(K1, rnd); rnd = mimc_hash(K2, rnd);                                                                     \
        for (int j = 0; j < batches; j++) rnd = mimc_hash(K3[j], rnd);                                                          \
        { oF x1 = rnd, x2 = f_mul(rnd, x1), x3 = f_mul(rnd, x2);                                                                \
          for (int j = 0; j < batches; j++) { Kp[j] = f_add(Kp[j], f_mul(rb[j][idx], K3[j])); Kf = f_add(Kf, f_mul(f_mul(x3, a[j]), K3[j])); } \
          Kf = f_add(Kf, f_add(f_mul(x2, K2), f_mul(x1, K1))); }                                                                \
        R[nR++] = rnd;                                                                                                          \
        for (int j = 0; j < batches; j++) { orc_fold_axpy(f1[j], b1[j], &rnd, sz[j]); orc_fold_axpy(f2[j], b2[j], &rnd, sz[j]); orc_fold_axpy(f3[j], b3[j], &rnd, sz[j]); } \
    } while (0)
#define LOAD_HALF(second) do { for (int j = 0; j < batches; j++) for (size_t k = 0; k < sz[j]; k++) {                          \
        b1[j][k] = V[j][2 * k + ((second) ? 2 * sz[j] : 0)]; b2[j][k] = V[j][2 * k + 1 + ((second) ? 2 * sz[j] : 0)]; } } while (0)
    LOAD_HALF(1); BATCH_PROD_STEP(half);
    for (size_t i = 1; i < nch; i++) {
        read_mul_tree_data(V, vlen, batches, 4 * B, layer_id, distance);
        LOAD_HALF(0); BATCH_PROD_STEP(i);
        LOAD_HALF(1); BATCH_PROD_STEP(i + half);
    }
    stream_reset();
    checks[0] = 1;
    for (int i = 0; i < n_old; i++) if (Kp[i].re != old_claims[i].re || Kp[i].im != old_claims[i].im) checks[0] = 0;
    /* P1 = batch_3product_sumcheck(fold_buff1, fold_buff2, fold_buff3, a) on concatenated tables */
    size_t tot = 0; for (int i = 0; i < batches; i++) tot += sz[i];
    oF *t1 = (oF *)malloc(sizeof(oF) * tot), *t2 = (oF *)malloc(sizeof(oF) * tot), *t3 = (oF *)malloc(sizeof(oF) * tot);
    { size_t o = 0; for (int i = 0; i < batches; i++) { memcpy(t1 + o, f1[i], sizeof(oF) * sz[i]); memcpy(t2 + o, f2[i], sizeof(oF) * sz[i]); memcpy(t3 + o, f3[i], sizeof(oF) * sz[i]); o += sz[i]; } }
    const int rounds1 = orc_batch_3product_sumcheck(t1, t2, t3, sz, batches, a, cpoly1, r1, vr1);
    { oF c = f_add(f_add(f_add(cpoly1[0], cpoly1[1]), f_add(cpoly1[2], cpoly1[3])), cpoly1[3]); checks[1] = (c.re == Kf.re && c.im == Kf.im); }
    /* Partial_Evals pass (:1315-1340) */
    oF *PE = (oF *)calloc(2 * (size_t)batches * nR, sizeof(oF));
    for (int k = 0; k < batches; k++) orc_precompute_beta(r1, (int)log2((double)sz[k]), b3[k]);          /* beta[k] (b3 reused) */
    for (size_t i = 0; i < nch; i++) {
        read_mul_tree_data(V, vlen, batches, 4 * B, layer_id, distance);
        for (int k = 0; k < batches; k++) {
            oF *p0 = PE + (size_t)(2 * k) * nR, *p1 = PE + (size_t)(2 * k + 1) * nR;
            for (size_t j = 0; j < vlen[k] / 4; j++) {
                p0[i] = f_add(p0[i], f_mul(b3[k][j], V[k][2 * j])); p0[i + nR / 2] = f_add(p0[i + nR / 2], f_mul(b3[k][j], V[k][2 * j + vlen[k] / 2]));
                p1[i] = f_add(p1[i], f_mul(b3[k][j], V[k][2 * j + 1])); p1[i + nR / 2] = f_add(p1[i + nR / 2], f_mul(b3[k][j], V[k][2 * j + 1 + vlen[k] / 2]));
            }
        }
    }
    /* permute_partial_evals (:1137-1148): only R is permuted (even entries, then odd) */
    oF *Rp = (oF *)malloc(sizeof(oF) * nR);
    for (size_t i = 0; i < nR / 2; i++) { Rp[i] = R[2 * i]; Rp[nR / 2 + i] = R[2 * i + 1]; }
    memcpy(R_out, Rp, sizeof(oF) * nR);
    oF bb[32]; orc_generate_randomness(2 * batches, bb);
    oF *ae = (oF *)calloc(nR, sizeof(oF));
    for (int i = 0; i < 2 * batches; i++) for (size_t j = 0; j < nR; j++) ae[j] = f_add(ae[j], f_mul(bb[i], PE[(size_t)i * nR + j]));
    oF zero = fint(0);
    orc_sumcheck2(Rp, ae, nR, &zero, qpoly2, r2, vr2, fin2);                                              /* previous_r = the never-updated local rand = F(0) */
    { oF sum = fint(0);
      for (int i = 0; i < batches; i++) { sum = f_add(sum, f_mul(bb[2 * i], vr1[3 * i])); sum = f_add(sum, f_mul(bb[2 * i + 1], vr1[3 * i + 1])); }
      oF c = f_add(f_add(qpoly2[0], qpoly2[1]), f_add(qpoly2[2], qpoly2[2])); checks[2] = (c.re == sum.re && c.im == sum.im); }
    const int lR = (int)log2((double)nR);
    const oF pad = fint((uint64_t)random());
    for (int i = 0; i < batches; i++) {
        oF *row = new_r + (size_t)i * new_r_ld; int n = 0;
        row[n++] = pad;
        for (int j = 0; j < logB - i * distance; j++) row[n++] = r1[j];
        for (int j = 0; j < lR; j++) row[n++] = r2[j];
        oF e0, e1; orc_evaluate_vector(PE + (size_t)(2 * i) * nR, nR, r2, lR, &e0); orc_evaluate_vector(PE + (size_t)(2 * i + 1) * nR, nR, r2, lR, &e1);
        new_claims[i] = f_add(f_mul(f_sub(fint(1), pad), e0), f_mul(pad, e1));
    }
    for (int i = 0; i < batches; i++) { free(f1[i]); free(f2[i]); free(f3[i]); free(b1[i]); free(b2[i]); free(b3[i]); free(rb[i]); free(V[i]); }
    free(R); free(Rp); free(t1); free(t2); free(t3); free(PE); free(ae);
    (void)rounds1;
    return (int)nR;
#undef BATCH_PROD_STEP
#undef LOAD_HALF
}


/* generate_claims_opt (src/sumcheck.cpp:1014-1054) */
void orc_generate_claims_opt(size_t fd_size, size_t B, const oF *r, int batches, int layer_id, int distance, oF *claims) {
    const size_t size = fd_size >> layer_id; const int logB = (int)log2((double)B);
    oF *beta[16], *rb[16], *V[16]; size_t vlen[16] = {0}, rbn[16] = {0};
    for (int i = 0; i < batches; i++) {
        const int n_init = logB - i * distance, n_rem = (int)log2((double)(size / 2)) - i * distance - n_init;
        vlen[i] = (4 * B) >> (i * distance); V[i] = (oF *)malloc(sizeof(oF) * vlen[i]);
        beta[i] = (oF *)malloc(sizeof(oF) * ((size_t)1 << n_init)); orc_precompute_beta(r, n_init, beta[i]);
        rbn[i] = (size_t)1 << n_rem; rb[i] = (oF *)malloc(sizeof(oF) * rbn[i]); orc_precompute_beta(r + n_init, n_rem, rb[i]);
        claims[i] = fint(0);
    }
    stream_reset();
    for (size_t i = 0; i < size / (4 * B); i++) {
        read_mul_tree_data(V, vlen, batches, 4 * B, layer_id, distance);
        for (int j = 0; j < batches; j++)
            for (size_t k = 0; k < vlen[j] / 4; k++) {
                claims[j] = f_add(claims[j], f_mul(f_mul(f_mul(rb[j][i], beta[j][k]), V[j][2 * k]), V[j][2 * k + 1]));
                claims[j] = f_add(claims[j], f_mul(f_mul(f_mul(rb[j][i + rbn[j] / 2], beta[j][k]), V[j][2 * k + vlen[j] / 2]), V[j][2 * k + 1 + vlen[j] / 2]));
            }
    }
    for (int i = 0; i < batches; i++) { free(beta[i]); free(rb[i]); free(V[i]); }
}

/* prove_gate_consistency (src/sumcheck.cpp:796-975) over a caller-supplied trace: chunk i = elements [i*B, (i+1)*B) of L, R, O (field
 * elements) and S (int selectors; 1 = addition gate), n_chunks = tr.size / BUFFER_SPACE.  read_trace itself belongs to the witness
 * generator (Seval / witness_stream.cpp) and is out of scope; NOT pinned against oracle/_ref as a whole for that reason -- its pieces are
 * (compute{2,3,4}p_error_terms: streamfold.npz; the degree-4 loop through prove_gate_consistency_standard: gate.npz; sumcheck2).
 * Outputs: R (n_chunks challenges, R[0] = 1), a (4), gate sumcheck transcript (poly: logB x 5, gr: logB), fin6 (the six folded values
 * add, beta, L, R, O, mul), Peval (6 x n_chunks), b (6), P (q2: lR x 3, r2, vr2, fin2).
 * checks: [0] "Error in gate consistency 1" held for every chunk, [1] "... 2" for every round, [2] "... 3". */
void orc_gate_consistency_stream(const oF *L, const oF *Rt, const oF *O, const int32_t *S, size_t n_chunks, size_t B, const oF *r, oF *R_out, oF *a_out, oF *poly, oF *gr,
                                 oF *fin6, oF *Peval, oF *b_out, oF *q2, oF *r2, oF *vr2, oF *fin2, int *checks) {
    const int logB = (int)log2((double)B);
    oF *beta = (oF *)malloc(sizeof(oF) * B), *fb = (oF *)malloc(sizeof(oF) * B), *fL = (oF *)malloc(sizeof(oF) * B), *fR = (oF *)malloc(sizeof(oF) * B),
       *fO = (oF *)malloc(sizeof(oF) * B), *fa = (oF *)malloc(sizeof(oF) * B), *fm = (oF *)malloc(sizeof(oF) * B);
    orc_precompute_beta(r, logB, beta); memcpy(fb, beta, sizeof(oF) * B);
    memcpy(fL, L, sizeof(oF) * B); memcpy(fR, Rt, sizeof(oF) * B); memcpy(fO, O, sizeof(oF) * B);
    for (size_t i = 0; i < B; i++) { fa[i] = fint((uint64_t)(int64_t)S[i]); fm[i] = f_sub(fint(1), fa[i]); }
    oF rnd = fint(0), KO = fint(0), KL = fint(0), KR = fint(0), KM = fint(0);
    for (size_t i = 0; i < B; i++) {
        KO = f_add(KO, f_mul(beta[i], fO[i])); KL = f_add(KL, f_mul(f_mul(beta[i], fL[i]), fa[i]));
        KR = f_add(KR, f_mul(f_mul(beta[i], fR[i]), fa[i])); KM = f_add(KM, f_mul(f_mul(f_mul(beta[i], fR[i]), fL[i]), fm[i]));
    }
    R_out[0] = fint(1); checks[0] = 1;
    for (size_t c = 1; c < n_chunks; c++) {
        const oF *bL = L + c * B, *bR = Rt + c * B, *bO = O + c * B; const int32_t *bS = S + c * B;
        oF K2[2] = {fint(0), fint(0)}, KLs[3] = {fint(0), fint(0), fint(0)}, KRs[3] = {fint(0), fint(0), fint(0)}, K4[4] = {fint(0), fint(0), fint(0), fint(0)};
        orc_err2p(bO, beta, fO, fb, B, K2);
        orc_err3p(bL, bS, fL, fa, fb, beta, B, KLs);
        orc_err3p(bR, bS, fR, fa, fb, beta, B, KRs);
        orc_err4p(bL, bR, beta, bS, fL, fR, fb, fm, B, K4);
        { oF t = f_sub(f_add(f_add(K4[3], KLs[2]), KRs[2]), K2[1]); if (!fis0(t)) checks[0] = 0; }
        rnd = mimc_hash(K2[0], rnd); rnd = mimc_hash(K2[1], rnd);
        rnd = mimc_hash(KLs[0], rnd); rnd = mimc_hash(KLs[1], rnd); rnd = mimc_hash(KLs[2], rnd);
        rnd = mimc_hash(KRs[0], rnd); rnd = mimc_hash(KRs[1], rnd); rnd = mimc_hash(KRs[2], rnd);
        R_out[c] = rnd;
        oF x1 = rnd, x2 = f_mul(rnd, x1), x3 = f_mul(rnd, x2), x4 = f_mul(rnd, x3);
        KO = f_add(KO, f_add(f_mul(x1, K2[0]), f_mul(x2, K2[1])));
        KL = f_add(KL, f_add(f_add(f_mul(x1, KLs[0]), f_mul(x2, KLs[1])), f_mul(x3, KLs[2])));
        KR = f_add(KR, f_add(f_add(f_mul(x1, KRs[0]), f_mul(x2, KRs[1])), f_mul(x3, KRs[2])));
        KM = f_add(KM, f_add(f_add(f_mul(x1, K4[0]), f_mul(x2, K4[1])), f_add(f_mul(x3, K4[2]), f_mul(x4, K4[3]))));
        for (size_t j = 0; j < B; j++) {
            oF s = fint((uint64_t)(int64_t)bS[j]);
            fa[j] = f_add(fa[j], f_mul(rnd, s)); fL[j] = f_add(fL[j], f_mul(rnd, bL[j])); fR[j] = f_add(fR[j], f_mul(rnd, bR[j]));
            fO[j] = f_add(fO[j], f_mul(rnd, bO[j])); fm[j] = f_add(fm[j], f_mul(rnd, f_sub(fint(1), s))); fb[j] = f_add(fb[j], f_mul(rnd, beta[j]));
        }
    }
    orc_generate_randomness(4, a_out);
    oF sum = f_add(f_add(f_mul(a_out[0], KL), f_mul(a_out[1], KR)), f_add(f_mul(a_out[2], KM), f_mul(KO, a_out[3])));
    orc_gate_sumcheck(fa, fb, fL, fR, fO, fm, B, a_out, &rnd, &sum, poly, gr, fin6, &checks[1]);
    /* Peval pass (:949-959) */
    oF *b1 = (oF *)malloc(sizeof(oF) * B);
    orc_precompute_beta(gr, logB, b1);
    for (size_t i = 0; i < 6 * n_chunks; i++) Peval[i] = fint(0);
    for (size_t c = 0; c < n_chunks; c++)
        for (size_t j = 0; j < B; j++) {
            oF s = fint((uint64_t)(int64_t)S[c * B + j]);
            Peval[0 * n_chunks + c] = f_add(Peval[0 * n_chunks + c], f_mul(b1[j], L[c * B + j]));
            Peval[1 * n_chunks + c] = f_add(Peval[1 * n_chunks + c], f_mul(b1[j], Rt[c * B + j]));
            Peval[2 * n_chunks + c] = f_add(Peval[2 * n_chunks + c], f_mul(b1[j], O[c * B + j]));
            Peval[3 * n_chunks + c] = f_add(Peval[3 * n_chunks + c], f_mul(b1[j], s));
            Peval[4 * n_chunks + c] = f_add(Peval[4 * n_chunks + c], f_mul(b1[j], f_sub(fint(1), s)));
            Peval[5 * n_chunks + c] = f_add(Peval[5 * n_chunks + c], f_mul(b1[j], beta[j]));
        }
    orc_generate_randomness(6, b_out);
    oF *pe = (oF *)calloc(n_chunks, sizeof(oF));
    for (size_t j = 0; j < n_chunks; j++) for (int i = 0; i < 6; i++) pe[j] = f_add(pe[j], f_mul(b_out[i], Peval[(size_t)i * n_chunks + j]));
    orc_sumcheck2(R_out, pe, n_chunks, &rnd, q2, r2, vr2, fin2);
    /* sum = fold_L[0]*b0 + fold_R[0]*b1 + fold_O[0]*b2 + b3*fold_add[0] + b4*fold_mul[0] + b5*fold_beta[0]; fin6 = add, beta, L, R, O, mul */
    { oF sm = f_add(f_add(f_mul(fin6[2], b_out[0]), f_mul(fin6[3], b_out[1])), f_add(f_mul(fin6[4], b_out[2]), f_mul(b_out[3], fin6[0])));
      sm = f_add(sm, f_add(f_mul(b_out[4], fin6[5]), f_mul(b_out[5], fin6[1])));
      oF c = f_add(f_add(q2[0], q2[1]), f_add(q2[2], q2[2])); checks[2] = (c.re == sm.re && c.im == sm.im); }
    free(beta); free(fb); free(fL); free(fR); free(fO); free(fa); free(fm); free(b1); free(pe);
}

/* prove_gate_consistency_lookups (src/sumcheck.cpp:503-795), the variant main.cpp:915 runs for circuits with lookup gates (has_lookups set),
 * over a caller-supplied trace as orc_gate_consistency_stream: selectors S in {0 addition, 1 multiplication, 2 lookup}; lr = lookup_rand[0..1].
 * The selector rewrites the reference does between its compute3p_error_terms calls (2 -> 3 -> 4, 0 -> -1 -> 0, :568-585) are restated
 * literally, with compute{3,4}p_error_terms's has_lookups gate maps (:388-394, :413-427).  Only K1_O .. K3_R enter the per-chunk transcript
 * (:596-603): the lookup and multiplication terms do not.  Unpinned as a whole for the same reason (read_trace is the witness generator's).
 * Outputs: R, a (5), poly (logB x 5), gr, fin9 (folded add_L, add_R, L, R, O, lkp, lkp_O, mul, beta: the order of :716-726),
 * Peval (8 x n_chunks), b (8), q2/r2/vr2/fin2.  checks: [0] "Error in gate consistency 1" per chunk incl. the initial one (:549),
 * [1] "... 2" per round, [2] "... 3", [3] the per-chunk Kf_M self-check (:635-641), [4] the Kf_lkp self-check (:646-652). */
static void err3p_lk(const oF *b1, const int32_t *sel, const oF *f1, const oF *f2, const oF *f3, const oF *beta, size_t n, const oF *lr, oF *K) {
    for (size_t j = 0; j < n; j++) {
        oF gate = lk_gate3(sel[j], lr);
        oF t1 = f_add(f_mul(b1[j], f2[j]), f_mul(gate, f1[j])), t2 = f_mul(b1[j], gate);
        K[0] = f_add(K[0], f_add(f_mul(f3[j], t1), f_mul(f_mul(beta[j], f1[j]), f2[j])));
        K[1] = f_add(K[1], f_add(f_mul(beta[j], t1), f_mul(f3[j], t2)));
        K[2] = f_add(K[2], f_mul(t2, beta[j]));
    }
}
static void err4p_lk(const oF *b1, const oF *b2, const oF *b3, const int32_t *sel, const oF *f1, const oF *f2, const oF *f3, const oF *f4, size_t n, oF *K) {
    for (size_t i = 0; i < n; i++) {
        oF gate = sel[i] == 1 ? fint(1) : fint(0);
        oF t1 = f_add(f_mul(f1[i], b2[i]), f_mul(f2[i], b1[i])), t2 = f_add(f_mul(f3[i], gate), f_mul(f4[i], b3[i]));
        oF t3 = f_mul(b1[i], b2[i]), t4 = f_mul(gate, b3[i]), t5 = f_mul(f1[i], f2[i]), t6 = f_mul(f3[i], f4[i]);
        K[0] = f_add(K[0], f_add(f_mul(t1, t6), f_mul(t2, t5)));
        K[1] = f_add(K[1], f_add(f_add(f_mul(t1, t2), f_mul(t3, t6)), f_mul(t4, t5)));
        K[2] = f_add(K[2], f_add(f_mul(t1, t4), f_mul(t2, t3)));
        K[3] = f_add(K[3], f_mul(t3, t4));
    }
}
static void cubic_acc(oF *c, oF b0, oF d0, oF b1, oF d1, oF b2, oF d2) {      /* (l1*l2)*l3, src/polynomial.cpp:91-93,133-135 */
    oF qa = f_mul(d0, d1), qb = f_add(f_mul(d0, b1), f_mul(b0, d1)), qc = f_mul(b0, b1);
    c[0] = f_add(c[0], f_mul(qa, d2));
    c[1] = f_add(c[1], f_add(f_mul(qa, b2), f_mul(qb, d2)));
    c[2] = f_add(c[2], f_add(f_mul(qb, b2), f_mul(qc, d2)));
    c[3] = f_add(c[3], f_mul(qc, b2));
}
void orc_gate_consistency_lookups_stream(const oF *L, const oF *Rt, const oF *O, const int32_t *S, size_t n_chunks, size_t B, const oF *r, const oF *lr, oF *R_out, oF *a_out,
                                         oF *poly, oF *gr, oF *fin9, oF *Peval, oF *b_out, oF *q2, oF *r2, oF *vr2, oF *fin2, int *checks) {
    const int logB = (int)log2((double)B);
    enum { AL, AR, TL, TR, TO, LK, LO, MU, BE };
    oF *t[9]; for (int q = 0; q < 9; q++) t[q] = (oF *)malloc(sizeof(oF) * B);
    oF *beta = (oF *)malloc(sizeof(oF) * B), *blo = (oF *)malloc(sizeof(oF) * B);
    int32_t *sel = (int32_t *)malloc(sizeof(int32_t) * B);
    orc_precompute_beta(r, logB, beta); memcpy(t[BE], beta, sizeof(oF) * B);
    memcpy(t[TL], L, sizeof(oF) * B); memcpy(t[TR], Rt, sizeof(oF) * B); memcpy(t[TO], O, sizeof(oF) * B);
    for (size_t i = 0; i < B; i++) {
        t[MU][i] = t[AL][i] = t[AR][i] = t[LK][i] = t[LO][i] = fint(0);
        if (S[i] == 0) { t[AL][i] = fint(1); t[AR][i] = fint(1); }
        else if (S[i] == 1) t[MU][i] = fint(1);
        else { t[AL][i] = lr[0]; t[AR][i] = lr[1]; t[LO][i] = f_sub(f_add(f_mul(lr[0], t[TL][i]), f_mul(lr[1], t[TR][i])), t[TO][i]); t[LK][i] = fint(1); }
    }
    oF rnd = fint(0), KO = fint(0), KL = fint(0), KR = fint(0), KM = fint(0), KK = fint(0);
    for (size_t i = 0; i < B; i++) {
        KO = f_add(KO, f_mul(beta[i], t[TO][i]));
        KL = f_add(KL, f_mul(f_mul(beta[i], t[TL][i]), t[AL][i]));
        KR = f_add(KR, f_mul(f_mul(beta[i], t[TR][i]), t[AR][i]));
        KK = f_add(KK, f_mul(f_mul(beta[i], t[LO][i]), t[LK][i]));
        KM = f_add(KM, f_mul(f_mul(f_mul(beta[i], t[TR][i]), t[TL][i]), t[MU][i]));
    }
    checks[0] = fis0(f_sub(f_sub(f_add(f_add(KM, KL), KR), KK), KO)); checks[3] = 1;
    R_out[0] = fint(1);
    for (size_t c = 1; c < n_chunks; c++) {
        const oF *bL = L + c * B, *bR = Rt + c * B, *bO = O + c * B;
        memcpy(sel, S + c * B, sizeof(int32_t) * B);
        oF K2[2] = {fint(0), fint(0)}, KLs[3] = {fint(0), fint(0), fint(0)}, KRs[3] = {fint(0), fint(0), fint(0)}, KKs[3] = {fint(0), fint(0), fint(0)},
           K4[4] = {fint(0), fint(0), fint(0), fint(0)};
        orc_err2p(bO, beta, t[TO], t[BE], B, K2);
        err3p_lk(bL, sel, t[TL], t[AL], t[BE], beta, B, lr, KLs);
        for (size_t j = 0; j < B; j++) if (sel[j] == 2) sel[j] = 3;
        err3p_lk(bR, sel, t[TR], t[AR], t[BE], beta, B, lr, KRs);
        for (size_t j = 0; j < B; j++) {
            blo[j] = fint(0);
            if (sel[j] == 0) sel[j] = -1;
            if (sel[j] == 3) { sel[j] = 4; blo[j] = f_sub(f_add(f_mul(lr[0], bL[j]), f_mul(lr[1], bR[j])), bO[j]); }
        }
        err3p_lk(blo, sel, t[LO], t[LK], t[BE], beta, B, lr, KKs);
        for (size_t j = 0; j < B; j++) if (sel[j] == -1) sel[j] = 0;
        err4p_lk(bL, bR, beta, sel, t[TL], t[TR], t[BE], t[MU], B, K4);
        { oF e = f_sub(f_sub(f_add(f_add(K4[3], KLs[2]), KRs[2]), KKs[2]), K2[1]); if (!fis0(e)) checks[0] = 0; }
        rnd = mimc_hash(K2[0], rnd); rnd = mimc_hash(K2[1], rnd);
        rnd = mimc_hash(KLs[0], rnd); rnd = mimc_hash(KLs[1], rnd); rnd = mimc_hash(KLs[2], rnd);
        rnd = mimc_hash(KRs[0], rnd); rnd = mimc_hash(KRs[1], rnd); rnd = mimc_hash(KRs[2], rnd);
        R_out[c] = rnd;
        oF x1 = rnd, x2 = f_mul(rnd, x1), x3 = f_mul(rnd, x2), x4 = f_mul(rnd, x3);
        KO = f_add(KO, f_add(f_mul(x1, K2[0]), f_mul(x2, K2[1])));
        KK = f_add(KK, f_add(f_add(f_mul(x1, KKs[0]), f_mul(x2, KKs[1])), f_mul(x3, KKs[2])));
        KL = f_add(KL, f_add(f_add(f_mul(x1, KLs[0]), f_mul(x2, KLs[1])), f_mul(x3, KLs[2])));
        KR = f_add(KR, f_add(f_add(f_mul(x1, KRs[0]), f_mul(x2, KRs[1])), f_mul(x3, KRs[2])));
        KM = f_add(KM, f_add(f_add(f_mul(x1, K4[0]), f_mul(x2, K4[1])), f_add(f_mul(x3, K4[2]), f_mul(x4, K4[3]))));
        for (size_t j = 0; j < B; j++) {
            if (sel[j] != 1) {
                if (sel[j] == 0) { t[AL][j] = f_add(t[AL][j], rnd); t[AR][j] = f_add(t[AR][j], rnd); }
                else { t[LK][j] = f_add(t[LK][j], rnd); t[AL][j] = f_add(t[AL][j], f_mul(rnd, lr[0])); t[AR][j] = f_add(t[AR][j], f_mul(rnd, lr[1])); }
            } else t[MU][j] = f_add(t[MU][j], rnd);
            t[TL][j] = f_add(t[TL][j], f_mul(rnd, bL[j])); t[TR][j] = f_add(t[TR][j], f_mul(rnd, bR[j])); t[TO][j] = f_add(t[TO][j], f_mul(rnd, bO[j]));
            t[LO][j] = f_add(t[LO][j], f_mul(rnd, blo[j])); t[BE][j] = f_add(t[BE][j], f_mul(rnd, beta[j]));
        }
        oF s = fint(0);
        for (size_t j = 0; j < B; j++) s = f_add(s, f_mul(f_mul(f_mul(t[BE][j], t[MU][j]), t[TR][j]), t[TL][j]));
        if (!(s.re == KM.re && s.im == KM.im)) checks[3] = 0;
    }
    orc_generate_randomness(5, a_out);
    { oF s = fint(0); for (size_t i = 0; i < B; i++) s = f_add(s, f_mul(f_mul(t[BE][i], t[LK][i]), t[LO][i])); checks[4] = (s.re == KK.re && s.im == KK.im); }
    const oF *a = a_out;
    oF sum = f_add(f_add(f_add(f_mul(a[0], KL), f_mul(a[1], KR)), f_add(f_mul(a[2], KM), f_mul(KO, a[3]))), f_mul(KK, a[4]));
    checks[1] = 1;
    for (int rd = 0, i = logB - 1; i >= 0; i--, rd++) {
        size_t Lh = (size_t)1 << i;
        oF c1[3][4], c4[5], c2[3];
        for (int q = 0; q < 3; q++) for (int k = 0; k < 4; k++) c1[q][k] = fint(0);
        for (int k = 0; k < 5; k++) c4[k] = fint(0);
        for (int k = 0; k < 3; k++) c2[k] = fint(0);
        for (size_t j = 0; j < Lh; j++) {
            oF b[9], d[9];
            for (int q = 0; q < 9; q++) { b[q] = t[q][2 * j]; d[q] = f_sub(t[q][2 * j + 1], b[q]); }
            cubic_acc(c1[0], b[AL], d[AL], b[BE], d[BE], b[TL], d[TL]);
            cubic_acc(c1[1], b[AR], d[AR], b[BE], d[BE], b[TR], d[TR]);
            cubic_acc(c1[2], b[LK], d[LK], b[BE], d[BE], b[LO], d[LO]);
            oF ma = f_mul(d[MU], d[BE]), mb = f_add(f_mul(d[MU], b[BE]), f_mul(b[MU], d[BE])), mc = f_mul(b[MU], b[BE]);
            oF ka = f_mul(ma, d[TL]), kb = f_add(f_mul(ma, b[TL]), f_mul(mb, d[TL])), kc = f_add(f_mul(mb, b[TL]), f_mul(mc, d[TL])), kd = f_mul(mc, b[TL]);
            c4[0] = f_add(c4[0], f_mul(ka, d[TR]));
            c4[1] = f_add(c4[1], f_add(f_mul(ka, b[TR]), f_mul(kb, d[TR])));
            c4[2] = f_add(c4[2], f_add(f_mul(kb, b[TR]), f_mul(kc, d[TR])));
            c4[3] = f_add(c4[3], f_add(f_mul(kc, b[TR]), f_mul(kd, d[TR])));
            c4[4] = f_add(c4[4], f_mul(kd, b[TR]));
            c2[0] = f_add(c2[0], f_mul(d[BE], d[TO]));
            c2[1] = f_add(c2[1], f_add(f_mul(d[BE], b[TO]), f_mul(b[BE], d[TO])));
            c2[2] = f_add(c2[2], f_mul(b[BE], b[TO]));
        }
        oF C[4], p[5];
        for (int k = 0; k < 4; k++) C[k] = f_add(f_add(f_mul(a[0], c1[0][k]), f_mul(a[1], c1[1][k])), f_mul(a[4], c1[2][k]));
        p[0] = f_mul(a[2], c4[0]);
        p[1] = f_add(f_mul(a[2], c4[1]), C[0]);
        p[2] = f_add(f_add(f_mul(a[2], c4[2]), C[1]), f_mul(a[3], c2[0]));
        p[3] = f_add(f_add(f_mul(a[2], c4[3]), C[2]), f_mul(a[3], c2[1]));
        p[4] = f_add(f_add(f_mul(a[2], c4[4]), C[3]), f_mul(a[3], c2[2]));
        for (int q = 0; q < 5; q++) { rnd = mimc_hash(p[q], rnd); poly[5 * rd + q] = p[q]; }
        oF s01 = f_add(f_add(f_add(p[0], p[1]), f_add(p[2], p[3])), f_add(p[4], p[4]));
        if (!(s01.re == sum.re && s01.im == sum.im)) checks[1] = 0;
        sum = f_add(f_mul(f_add(f_mul(f_add(f_mul(f_add(f_mul(p[0], rnd), p[1]), rnd), p[2]), rnd), p[3]), rnd), p[4]);
        gr[rd] = rnd;
        for (size_t j = 0; j < Lh; j++) for (int q = 0; q < 9; q++) t[q][j] = f_add(t[q][2 * j], f_mul(rnd, f_sub(t[q][2 * j + 1], t[q][2 * j])));
    }
    for (int q = 0; q < 9; q++) fin9[q] = t[q][0];
    /* Peval pass (:741-764) */
    oF *b1 = (oF *)malloc(sizeof(oF) * B);
    orc_precompute_beta(gr, logB, b1);
    for (size_t i = 0; i < 8 * n_chunks; i++) Peval[i] = fint(0);
    for (size_t c = 0; c < n_chunks; c++)
        for (size_t j = 0; j < B; j++) {
            const size_t g = c * B + j;
            oF *P = Peval + c;
            P[0 * n_chunks] = f_add(P[0 * n_chunks], f_mul(b1[j], L[g]));
            P[1 * n_chunks] = f_add(P[1 * n_chunks], f_mul(b1[j], Rt[g]));
            P[2 * n_chunks] = f_add(P[2 * n_chunks], f_mul(b1[j], O[g]));
            if (S[g] == 0) { P[3 * n_chunks] = f_add(P[3 * n_chunks], b1[j]); P[4 * n_chunks] = f_add(P[4 * n_chunks], b1[j]); }
            else if (S[g] == 1) P[5 * n_chunks] = f_add(P[5 * n_chunks], b1[j]);
            else {
                P[3 * n_chunks] = f_add(P[3 * n_chunks], f_mul(b1[j], lr[0])); P[4 * n_chunks] = f_add(P[4 * n_chunks], f_mul(b1[j], lr[1]));
                P[6 * n_chunks] = f_add(P[6 * n_chunks], b1[j]);
                P[7 * n_chunks] = f_add(P[7 * n_chunks], f_mul(b1[j], f_sub(f_add(f_mul(lr[0], L[g]), f_mul(lr[1], Rt[g])), O[g])));
            }
        }
    orc_generate_randomness(8, b_out);
    oF *pe = (oF *)calloc(n_chunks, sizeof(oF));
    for (size_t j = 0; j < n_chunks; j++) for (int i = 0; i < 8; i++) pe[j] = f_add(pe[j], f_mul(b_out[i], Peval[(size_t)i * n_chunks + j]));
    orc_sumcheck2(R_out, pe, n_chunks, &rnd, q2, r2, vr2, fin2);
    {   /* (:783-789) */
        oF sm = f_add(f_add(f_mul(fin9[TL], b_out[0]), f_mul(fin9[TR], b_out[1])), f_mul(fin9[TO], b_out[2]));
        sm = f_add(sm, f_mul(b_out[3], fin9[AL])); sm = f_add(sm, f_mul(b_out[4], fin9[AR])); sm = f_add(sm, f_mul(b_out[5], fin9[MU]));
        sm = f_add(sm, f_mul(b_out[6], fin9[LK])); sm = f_add(sm, f_mul(b_out[7], fin9[LO]));
        oF c = f_add(f_add(q2[0], q2[1]), f_add(q2[2], q2[2])); checks[2] = (c.re == sm.re && c.im == sm.im);
    }
    for (int q = 0; q < 9; q++) free(t[q]);
    free(beta); free(blo); free(sel); free(b1); free(pe);
}

/* Elastic_PC commit (RS x RS) of a "PC_layer" stream (commit_layers, src/sumcheck.cpp:983-1003): read_stream_PC's PC_layer branch
 * (src/witness_stream.cpp:2357-2364) hands read_mul_tree_layer the descriptor itself, whose name no branch of read_stream knows -- so
 * every chunk is the product layer `layer` of the DEFAULT stream (not of the stream the tree is about: the reference as it is). */
size_t orc_elastic_commit_pc_layer(size_t N, size_t B, int layer, uint8_t *levels_out) {
    const int trs = (int)(B >> 11);
    size_t T = 4 * B;
    oF *buff = (oF *)malloc(sizeof(oF) * B), *tensor = (oF *)malloc(sizeof(oF) * T);
    oF *ci[3]; for (int i = 0; i < 3; i++) ci[i] = (oF *)malloc(sizeof(oF) * T);
    memset(levels_out, 0, 32 * T);
    for (size_t i = 0; i < N / B; i++) {
        stream_reset(); read_mul_tree_layer(buff, B, layer);
        orc_compute_tensorcode(buff, B, trs, 0, tensor);
        if (i % 4 != 3) memcpy(ci[i % 4], tensor, sizeof(oF) * T);
        else for (size_t p = 0; p < T; p++) {
            oF z = fint(0);
            oF xx[4] = {p + 1 < T ? ci[0][p + 1] : z, p + 1 < T ? ci[1][p + 1] : z, ci[2][p], tensor[p]};
            hash_md(xx, levels_out + 32 * p, levels_out + 32 * p);
        }
    }
    free(buff); free(tensor); for (int i = 0; i < 3; i++) free(ci[i]);
    return create_tree(levels_out, T);
}

/* Multi-GPU streaming commit (test infra for tests/test_dist_gloo.py): the inner digests H(c0[p+1], c1[p+1], c2[p], t3[p]) of ONE group of
 * 4 consecutive chunks, 4B x 32 B in leaf order, exactly what orc_elastic_commit chains -- chunk c of the stream under the stream model
 * (kind 0: every chunk is read_stream_PC's default; kind 1: chunk c = splitmix_field(B, seed + c)). */
void orc_elastic_group_digests(size_t B, int opt, size_t group, uint8_t *out) {
    int lin, trs;
    if (opt == 1) { lin = 0; trs = (int)(B >> 11); } else { lin = 1; trs = (int)(B >> 14); }
    size_t T = 4 * B;
    oF *buff = (oF *)malloc(sizeof(oF) * B), *t[4];
    const uint64_t save = g_stream_count;
    for (int q = 0; q < 4; q++) {
        t[q] = (oF *)malloc(sizeof(oF) * T);
        if (g_stream_kind == 0) orc_read_stream_pc(B, buff); else { g_stream_count = 4 * group + (size_t)q; stream_read(buff, B); }
        orc_compute_tensorcode(buff, B, trs, lin, t[q]);
    }
    g_stream_count = save;
    for (size_t p = 0; p < T; p++) {
        oF z = fint(0);
        oF x[4] = {p + 1 < T ? t[0][p + 1] : z, p + 1 < T ? t[1][p + 1] : z, t[2][p], t[3][p]};
        blake3_64((const uint8_t *)x, out + 32 * p);
    }
    free(buff); for (int q = 0; q < 4; q++) free(t[q]);
}
/* the whole streaming commit under the stream model (kind 1: chunk c = splitmix_field(B, seed + c)); graphs must already be drawn for opt 2 */
size_t orc_elastic_commit_model(size_t N, size_t B, int opt, uint8_t *levels_out) {
    size_t T = 4 * B, groups = N / T;
    uint8_t *dg = (uint8_t *)malloc(32 * T);
    memset(levels_out, 0, 32 * T);
    for (size_t g = 0; g < groups; g++) {
        orc_elastic_group_digests(B, opt, g, dg);
        for (size_t p = 0; p < T; p++) { uint8_t blk[64]; memcpy(blk, dg + 32 * p, 32); memcpy(blk + 32, levels_out + 32 * p, 32); blake3_64(blk, levels_out + 32 * p); }
    }
    free(dg);
    return create_tree(levels_out, T);
}

/* test_PC(N, 4, K) inputs (src/Our_PC.cpp:757-813) + timed commit_standard */
double orc_time_commit_standard(size_t N, int K) {
    srandom(1);
    oF *poly = (oF *)malloc(sizeof(oF) * N);
    orc_generate_randomness((int)N, poly);
    int trs = (int)(N / ((size_t)K << 11));
    orc_expander_init_store(trs);
    size_t M = N / (size_t)K;
    uint8_t *lv = (uint8_t *)malloc(64 * M);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    orc_commit_standard(poly, N, K, trs, 1, lv, NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    free(poly); free(lv);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}

/* ------------------------------------------------------------------------------------------ */
/* The same commit_standard on T threads (the "all host cores" CPU leg).    */
/* Chunk after chunk as above; inside a chunk the rows (FFT), then the columns (encode), then   */
/* the leaves (hash chain step) are dealt to the threads in contiguous ranges, with a barrier   */
/* between the three loops.  Same arithmetic in the same order per element: same levels.        */
/* ------------------------------------------------------------------------------------------ */
#include <pthread.h>
typedef struct { const oF *poly; size_t M, cols, rows; int K, trs, lin, T, id; oF *t; uint8_t *levels; oF *tensor_out; pthread_barrier_t *bar; } mt_arg;
static void *mt_worker(void *p) {
    mt_arg *a = (mt_arg *)p;
    const size_t trs = (size_t)a->trs, cols = a->cols, rows = a->rows, half = a->M / trs;
    const int logc = (int)log2((double)cols), logr = (int)log2((double)rows);
    oF *buf = (oF *)malloc(sizeof(oF) * rows), *buf2 = (oF *)malloc(sizeof(oF) * rows);
    for (int i = 0; i < a->K; i++) {
        const oF *msg = a->poly + (size_t)i * a->M;
        size_t lo = trs * (size_t)a->id / (size_t)a->T, hi = trs * (size_t)(a->id + 1) / (size_t)a->T;
        for (size_t r = lo; r < hi; r++) {                                   /* message rows: copy, zero-pad, row FFT */
            memcpy(a->t + r * cols, msg + r * half, sizeof(oF) * half);
            memset(a->t + r * cols + half, 0, sizeof(oF) * (cols - half));
            orc_fft_cached(a->t + r * cols, logc, 0);
        }
        pthread_barrier_wait(a->bar);
        lo = cols * (size_t)a->id / (size_t)a->T; hi = cols * (size_t)(a->id + 1) / (size_t)a->T;
        for (size_t c = lo; c < hi; c++) {
            if (!a->lin) {
                for (size_t j = 0; j < rows; j++) buf[j] = j < trs ? a->t[j * cols + c] : fint(0);
                orc_fft_cached(buf, logr, 0);
                for (size_t j = 0; j < rows; j++) a->t[j * cols + c] = buf[j];
            } else {
                for (size_t j = 0; j < trs; j++) buf[j] = a->t[j * cols + c];
                orc_encode_monolithic(buf, buf2, (long long)trs);
                for (size_t j = 0; j < rows; j++) a->t[j * cols + c] = buf2[j];
            }
        }
        pthread_barrier_wait(a->bar);
        if (a->tensor_out && a->id == 0) memcpy(a->tensor_out + (size_t)i * rows * cols, a->t, sizeof(oF) * rows * cols);
        const size_t nl = trs / 2 * cols;
        lo = nl * (size_t)a->id / (size_t)a->T; hi = nl * (size_t)(a->id + 1) / (size_t)a->T;
        for (size_t g = lo; g < hi; g++) {
            const size_t j = g / cols, k = g % cols;
            oF x[4] = {a->t[(4 * j) * cols + k], a->t[(4 * j + 1) * cols + k], a->t[(4 * j + 2) * cols + k], a->t[(4 * j + 3) * cols + k]};
            uint8_t *leaf = a->levels + 32 * g;
            hash_md(x, leaf, leaf);
        }
        pthread_barrier_wait(a->bar);
    }
    free(buf); free(buf2);
    return NULL;
}
size_t orc_commit_standard_mt(const oF *poly, size_t N, int K, int trs, int lin, int T, uint8_t *levels_out, oF *tensor_out) {
    size_t M = N / (size_t)K, cols = 2 * M / (size_t)trs, rows = 2 * (size_t)trs;
    if (T < 1) T = 1;
    if ((size_t)T > (size_t)trs) T = trs;
    oF *t = (oF *)malloc(sizeof(oF) * rows * cols);
    memset(levels_out, 0, 32 * M);
    /* the twiddle cache is keyed on the length only (quirk above) and is not thread-safe to fill: with RS x RS the two lengths would
       thrash it, so that mode runs on one thread; RS x expander uses one length, filled here before the workers start */
    if (!lin) T = 1;
    { oF *one = (oF *)calloc(cols, sizeof(oF)); orc_fft_cached(one, (int)log2((double)cols), 0); free(one); }
    pthread_barrier_t bar; pthread_barrier_init(&bar, NULL, (unsigned)T);
    pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)T); mt_arg *args = (mt_arg *)malloc(sizeof(mt_arg) * (size_t)T);
    for (int i = 0; i < T; i++) {
        args[i] = (mt_arg){poly, M, cols, rows, K, trs, lin, T, i, t, levels_out, tensor_out, &bar};
        pthread_create(&th[i], NULL, mt_worker, &args[i]);
    }
    for (int i = 0; i < T; i++) pthread_join(th[i], NULL);
    pthread_barrier_destroy(&bar); free(th); free(args); free(t);
    return create_tree(levels_out, M);
}
double orc_time_commit_standard_mt(size_t N, int K, int T) {
    srandom(1);
    oF *poly = (oF *)malloc(sizeof(oF) * N);
    orc_generate_randomness((int)N, poly);
    int trs = (int)(N / ((size_t)K << 11));
    orc_expander_init_store(trs);
    size_t M = N / (size_t)K;
    uint8_t *lv = (uint8_t *)malloc(64 * M);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    orc_commit_standard_mt(poly, N, K, trs, 1, T, lv, NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    free(poly); free(lv);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
