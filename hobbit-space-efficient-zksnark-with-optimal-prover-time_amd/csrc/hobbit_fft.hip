// hobbit_fft.hip -- the FFT of every scheme: the gfx950 kernels and their launchers, the twiddle-table cache, the dispatch by length, and
// the two FFT entry points of the C ABI.  hobbit_fft.hpp is all that the rest of the library sees of it.
#include "hobbit_fft.hpp"
#include "hobbit_dev.hpp"
#include "hobbit_fft_tables.hpp"
#include "hobbit_kernels.hpp"
#include "hobbit_rot.hpp"
#include "hobbit_half.hpp"
#include "../../include/hobbit_real.h"
#include "../../include/hobbit_elastic_real.h"
#include "../../include/hobbit_real_rs.h"

namespace hobbit {
// ============================================================================================
// FFT: one workgroup per row, the whole row (<= 4096 x 16 B = 64 KB) in LDS.
// Radix-2 DIT on bit-reversed input == the reference's _fft (src/utils.cpp:605-673): same DFT,
// natural order in and out.  Two radix-2 stages are fused per barrier (radix-4 in registers).
// The source row may be shorter than the transform (zero padding, src/PC_utils.cpp:75-84) and the
// destination may be strided (dst_es = element stride), which is how the row FFT of the tensor
// code writes straight into the codeword-major tensor.
// ============================================================================================
// Short transforms (len < 1024) are packed: a workgroup owns tpw = 1024 / len consecutive rows, so that every radix-4 stage still
// has one butterfly per thread (a single 256-point row would keep one wave of four busy).
// The stages themselves, on `span / len` bit-reversed rows held in LDS.  Element i of a row sits at slot i + i/8 (one pad per eight):
// the stride-4 and stride-16 butterflies of the first two radix-4 stages then spread over all banks (a plain layout is 4-way
// conflicted there); the row stride ldr must be >= fft_row_slots(len).
__device__ __host__ __forceinline__ uint32_t fft_slot(uint32_t i) { return i + (i >> 3); }
__device__ __host__ __forceinline__ uint32_t fft_row_slots(uint32_t len) { return len + (len >> 3); }
__device__ __forceinline__ void fft_lds_stages(F *s, int logn, const F *__restrict__ tw, uint32_t span, uint32_t ldr) {
    const uint32_t len = 1u << logn;
    uint32_t h = 1;
    int st = 0;
    if (logn & 1) {   // single radix-2 stage first when the stage count is odd
        for (uint32_t g = threadIdx.x; g < span / 2; g += blockDim.x) {
            const uint32_t base = (g >> (logn - 1)) * ldr, i = 2 * (g & (len / 2 - 1));
            F u = ldF(&s[base + fft_slot(i)]), v = ldF(&s[base + fft_slot(i + 1)]);   // twiddle w^0 = 1
            stF(&s[base + fft_slot(i)], fadd(u, v)); stF(&s[base + fft_slot(i + 1)], fsub(u, v));
        }
        __syncthreads();
        h = 2; st = 1;
    }
    for (; st < logn; st += 2, h <<= 2) {
        const uint32_t sA = len / (2 * h), sB = len / (4 * h);   // twiddle strides of the two stages
        for (uint32_t g = threadIdx.x; g < span / 4; g += blockDim.x) {
            const uint32_t t = g >> (logn - 2), b = g & (len / 4 - 1);
            const uint32_t k = b & (h - 1), j = b / h;
            const uint32_t base = t * ldr, i0 = j * 4 * h + k;
            const uint32_t p0 = base + fft_slot(i0), p1 = base + fft_slot(i0 + h), p2 = base + fft_slot(i0 + 2 * h), p3 = base + fft_slot(i0 + 3 * h);
            F a0 = ldF(&s[p0]), a1 = ldF(&s[p1]), a2 = ldF(&s[p2]), a3 = ldF(&s[p3]);
            const F wA = ldF(tw + (size_t)k * sA);
            F t1 = fmul(a1, wA), t3 = fmul(a3, wA);
            F b0 = fadd(a0, t1), b1 = fsub(a0, t1), b2 = fadd(a2, t3), b3 = fsub(a2, t3);
            const F wB0 = ldF(tw + (size_t)k * sB), wB1 = ldF(tw + (size_t)(k + h) * sB);
            F u2 = fmul(b2, wB0), u3 = fmul(b3, wB1);
            stF(&s[p0], fadd(b0, u2)); stF(&s[p2], fsub(b0, u2));
            stF(&s[p1], fadd(b1, u3)); stF(&s[p3], fsub(b1, u3));
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256)
k_fft_rows(const F *__restrict__ src, size_t src_ld, uint32_t src_len, F *__restrict__ dst, size_t dst_ld, size_t dst_es,
           int logn, const F *__restrict__ tw, F scale, int do_scale, uint32_t rows_per_group, size_t src_gs, size_t dst_gs, uint32_t total_rows,
           uint32_t tpw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    const uint32_t len = 1u << logn;
    const uint32_t row0 = blockIdx.x * tpw, nrows = min(tpw, total_rows - row0), span = nrows * len, ldr = fft_row_slots(len);
    // row = (group, r): lets one launch cover K chunks x trs rows with per-chunk base strides
    for (uint32_t e = threadIdx.x; e < span; e += blockDim.x) {
        const uint32_t t = e >> logn, i = e & (len - 1), row = row0 + t;
        const F *in = src + (size_t)(row / rows_per_group) * src_gs + (size_t)(row % rows_per_group) * src_ld;
        F v = i < src_len ? ldF(in + i) : fmake(0);
        stF(&s[t * ldr + fft_slot(__brev(i) >> (32 - logn))], v);
    }
    __syncthreads();
    fft_lds_stages(s, logn, tw, span, ldr);
    for (uint32_t e = threadIdx.x; e < span; e += blockDim.x) {
        const uint32_t t = e >> logn, i = e & (len - 1), row = row0 + t;
        F *out = dst + (size_t)(row / rows_per_group) * dst_gs + (size_t)(row % rows_per_group) * dst_ld;
        F v = ldF(&s[t * ldr + fft_slot(i)]);
        if (do_scale) v = fmul(v, scale);
        stF(out + (size_t)i * dst_es, v);
    }
}
// The second half of a long transform len = 4096 R in ONE pass (was: twiddle + transpose, 4096 x FFT-R, transpose).  Input
// y[n1][k2] (R rows of 4096: the R sub-transforms), output X[k1 * 4096 + k2] = sum_n1 W_R^(n1 k1) W_len^(n1 k2) y[n1][k2].
// A workgroup owns C = 16 adjacent k2 for all n1: loads and stores are 256-byte segments, the twiddles come from the 2-D table
// tw2[n1][k2] with the same pattern, each of the C columns is one length-R transform in LDS (row stride odd: the column-major
// fill and drain are bank-conflict-free).
// SCALE: every result leaves multiplied by `scale` (the inverse transform's 1/len); the forward instantiation is the kernel as it was.
template <bool SCALE>
__global__ void __launch_bounds__(512)
k_fft_cols(const F *__restrict__ y, size_t gs, int logr, F *__restrict__ out, const F *__restrict__ tw2, const F *__restrict__ twr, F scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    constexpr uint32_t C = 16;
    const uint32_t R = 1u << logr, ldr = fft_row_slots(R) + 1, k20 = blockIdx.x * C;
    const F *src = y + (size_t)blockIdx.y * gs;
    F *dst = out + (size_t)blockIdx.y * gs;
    for (uint32_t e = threadIdx.x; e < C * R; e += blockDim.x) {
        const uint32_t n1 = e / C, t = e % C;
        const size_t at = (size_t)n1 * 4096 + k20 + t;
        F v = ldF(src + at);
        if (n1) v = fmul(v, ldF(tw2 + at));                               // W_len^(n1 k2); row 0 of the table is all ones
        stF(&s[t * ldr + fft_slot(__brev(n1) >> (32 - logr))], v);
    }
    __syncthreads();
    fft_lds_stages(s, logr, twr, C * R, ldr);
    for (uint32_t e = threadIdx.x; e < C * R; e += blockDim.x) {
        const uint32_t k1 = e / C, t = e % C;
        F v = ldF(&s[t * ldr + fft_slot(k1)]);
        if (SCALE) v = fmul(v, scale);
        stF(dst + (size_t)k1 * 4096 + k20 + t, v);
    }
}
static int launch_fft_cols(hobbit_ctx *ctx, const F *y, size_t gs, int logr, F *out, const F *tw2, const F *twr, F scale, int do_scale, uint32_t batch) {
    if (logr < 2 || logr > 4) return ctx->fail(HOBBIT_EINVAL, "fft_cols: R must be in [4, 16]");      // (R = 32 .. 256: k_fft_cols_r8)
    const size_t lds = (size_t)16 * (fft_row_slots(1u << logr) + 1) * 16;                              // at most 4.75 KB: under the default limit
    if (do_scale) { HB_LAUNCH(ctx, "k_fft_cols", k_fft_cols<true>, dim3(4096 / 16, batch), dim3(512), lds, y, gs, logr, out, tw2, twr, scale); }
    else { HB_LAUNCH(ctx, "k_fft_cols", k_fft_cols<false>, dim3(4096 / 16, batch), dim3(512), lds, y, gs, logr, out, tw2, twr, scale); }
    return 0;
}

static int launch_fft_rows(hobbit_ctx *ctx, const F *src, size_t src_ld, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es,
                    int logn, const F *tw, F scale, int do_scale, uint32_t groups, uint32_t rows_per_group, size_t src_gs, size_t dst_gs) {
    if (logn < 1 || logn > 12) return ctx->fail(HOBBIT_EINVAL, "fft: logn must be in [1,12] for the LDS-resident kernel");
    static std::atomic<uint64_t> attr_set{0};
    set_lds_limit_once(ctx, (const void *)k_fft_rows, 81920, attr_set);
    const size_t total = (size_t)groups * rows_per_group;
    if (total == 0) return 0;
    if (total >> 32) return ctx->fail(HOBBIT_EINVAL, "fft: too many rows");
    const uint32_t tpw = logn < 10 ? (1024u >> logn) : 1u;
    const size_t lds = (size_t)16 * fft_row_slots(1u << logn) * tpw;
    const size_t blocks = (total + tpw - 1) / tpw;
    HB_LAUNCH(ctx, "k_fft_rows", k_fft_rows, dim3((unsigned)blocks), dim3(256), lds, src, src_ld, src_len, dst, dst_ld, dst_es, logn, tw,
              scale, do_scale, rows_per_group, src_gs, dst_gs, (uint32_t)total, tpw);
    return 0;
}

// --------------------------------------------------------------------------------------------
// FFT-4096, the hot size (row RS-encode of every tensor code): 512 threads, radix-8 DIT in
// registers, four passes, LDS padded by one slot per eight (phys(i) = i + i/8) so that the
// stride-8 / stride-64 / stride-512 butterflies and the bit-reversed first-pass gather are all
// bank-conflict-free; 73.7 KB of LDS -> two workgroups per CU.
//   load     global -> LDS in natural order (coalesced, contiguous LDS writes)
//   pass 0   butterfly b reads x[rev9(b) + 512 u]  (= DIT positions 8b+t), writes positions 8b+t.
//            Its twiddles are the 8th roots of unity: 1, w4 = +-i (free), w8, w8^3; with the
//            zero-padded message rows (upper half 0) the first stage has no arithmetic at all.
//   pass 1,2 in place, twiddle tables stored per pass as [7][h] (contiguous in k)
//   pass 3   results go straight to global memory (row-major or codeword-major/transposed)
// Same DFT as the reference's _fft (src/utils.cpp:605-673): bit-exact by exactness of F_{p^2}.
// --------------------------------------------------------------------------------------------
struct Fft4kConst { F w8, w8_3; int w4_plus_i; };

// Inside the transform the sums are lazy.  p = 2^61 - 1 leaves three spare bits in a 64-bit word (8p + 7 = 2^64 - 1), exactly the
// growth of the three add/sub levels of an 8-point DFT: a + b is a plain 64-bit add, a - b is a + (B p - b) with B p the static bound of
// b, and every output is folded once (mask / shift / add) into [0, p + 7] -- 16 folds per octet instead of 48.  Bounds: the octet's
// first element comes from LDS in [0, p + 7], the other seven are products (canonical, < p); the first element is always the left
// operand of its butterflies, so the +7 only rides along: level 1 <= 2p + 7, level 2 <= 4p + 7, level 3 <= 8p + 7.
// (Same-box A/B at 2^28: 5.56 vs 6.04 ms for the zero-padded rows, 6.26 vs 6.74 ms for full rows.)
__device__ __forceinline__ uint64_t fold61(uint64_t s) { return (s & P61) + (s >> 61); }            // any u64 -> [0, p + 7], same residue
__device__ __forceinline__ F ffold(const F &a) { return fmake(fold61(a.re), fold61(a.im)); }
__device__ __forceinline__ F fcanon(const F &a) {                                                    // any u64 pair -> canonical
    const uint64_t r = fold61(a.re), i = fold61(a.im);
    return fmake(r >= P61 ? r - P61 : r, i >= P61 ? i - P61 : i);
}
__device__ __forceinline__ F faddl(const F &a, const F &b) { return fmake(a.re + b.re, a.im + b.im); }
template <int B> __device__ __forceinline__ F fsubl(const F &a, const F &b) {                       // b's components <= B p
    return fmake(a.re + ((uint64_t)B * P61 - b.re), a.im + ((uint64_t)B * P61 - b.im));
}
// a * b for a lazy a (components < 2^62 - 2^10) and a canonical twiddle b.  Same Karatsuba form as fmul, with the offset that keeps
// ac - bd non-negative doubled: C = p 2^62 >= bd, ac + C < 2^124, ad + bc < 2^124.
#if !defined(HOBBIT_FMUL_U128)
// (the carry-free limb product of hobbit_field.hpp takes components up to p + 7 -- what ffold leaves -- and its canonical form is what the octet's
// bounds need for the seven right-hand operands)
__device__ __forceinline__ F fmul_lz(const F &a, const F &b) { return fmul(a, b); }
#else
__device__ __forceinline__ F fmul_lz(const F &a, const F &b) {
    const u128 ac = (u128)a.re * b.re, bd = (u128)a.im * b.im;
    const u128 all = (u128)(a.re + a.im) * (b.re + b.im);
    const u128 C = ((u128)P61) << 62;
    return fmake(red124(ac + C - bd), red124(all - ac - bd));
}
#endif
template <int B> __device__ __forceinline__ F fmul_w4(const F &a, int plus_i) {   // a * (+i) or a * (-i); components <= B p in and out
    return plus_i ? fmake((uint64_t)B * P61 - a.im, a.re) : fmake(a.im, (uint64_t)B * P61 - a.re);
}
// a * w8, w8 = the primitive 8th root of unity of the transform direction.  sqrt(2) = 2^31 in F_p (2^62 = 2), so
// w8 = 2^30 (1 - i) forward (w4 = -i) and 2^30 (1 + i) inverse: a rotation by 30 bits of (a.re +- a.im), no product at all.
__device__ __forceinline__ uint64_t rot30(uint64_t x) {      // x * 2^30 mod p for any u64 x; result < 2^61 + 2^31 <= 2p
    x = fold61(x);                                           // < 2^62: x = lo31 + hi 2^31, x 2^30 = lo31 2^30 + hi (2^61 = 1)
    return ((x << 30) & P61) + (x >> 31);
}
template <int B> __device__ __forceinline__ F fmul_w8(const F &a, int plus_i) {   // components <= B p (B <= 4) in, <= 2p out
    const uint64_t s = a.re + a.im;
    return plus_i ? fmake(rot30(a.re + ((uint64_t)B * P61 - a.im)), rot30(s)) : fmake(rot30(s), rot30(a.im + ((uint64_t)B * P61 - a.re)));
}
__device__ __forceinline__ uint32_t fft_phys(uint32_t i) { return i + (i >> 3); }
#define HB_BFLY(x, y, w) do { F v__ = fmul(y, w); y = fsub(x, v__); x = fadd(x, v__); } while (0)
#define HB_BFLYL(B, x, y) do { F v__ = y; y = fsubl<B>(x, v__); x = faddl(x, v__); } while (0)      /* y <= B p */
// first stage of the 8-point DIT DFT: right operands canonical
#define HB_DFT8_HEAD(a) do { HB_BFLYL(1, a[0], a[1]); HB_BFLYL(1, a[2], a[3]); HB_BFLYL(1, a[4], a[5]); HB_BFLYL(1, a[6], a[7]); } while (0)
// the last two stages of an 8-point DIT DFT on a[0..7] (inputs in bit-reversed order, first stage done): twiddles 1, w4, w8, w8^3.
// In: a[0], a[1] <= 2p + 7, the rest <= 2p.  Out: <= 8p + 7 = 2^64 - 1, unfolded.
__device__ __forceinline__ void dft8_tail(F (&a)[8], int plus_i) {
    F t;
    HB_BFLYL(2, a[0], a[2]);
    t = fmul_w4<2>(a[3], plus_i); a[3] = fsubl<2>(a[1], t); a[1] = faddl(a[1], t);
    HB_BFLYL(2, a[4], a[6]);
    t = fmul_w4<2>(a[7], plus_i); a[7] = fsubl<2>(a[5], t); a[5] = faddl(a[5], t);
    // left operands a[0..3] <= 4p + 7, right operands a[4..7] <= 4p
    HB_BFLYL(4, a[0], a[4]);
    t = fmul_w8<4>(a[5], plus_i); a[5] = fsubl<2>(a[1], t); a[1] = faddl(a[1], t);
    t = fmul_w4<4>(a[6], plus_i); a[6] = fsubl<4>(a[2], t); a[2] = faddl(a[2], t);
    t = fmul_w4<2>(fmul_w8<4>(a[7], plus_i), plus_i); a[7] = fsubl<2>(a[3], t); a[3] = faddl(a[3], t);
}

template <bool PADDED>
__global__ void __launch_bounds__(512)
k_fft4096(const F *__restrict__ src, size_t src_ld, size_t src_es, F *__restrict__ dst, size_t dst_ld, size_t dst_es, const F *__restrict__ tw1,
          const F *__restrict__ tw2, const F *__restrict__ tw3, Fft4kConst cst, F scale, int do_scale, uint32_t rows_per_group, size_t src_gs,
          size_t dst_gs, int line_remap, uint32_t rot_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    // Transposed stores (dst_ld == 1): row r's element lands 16 B into the 128-byte line it shares with rows 8g .. 8g+7.  Workgroups b, b+8,
    // b+16, ... share an XCD and its L2, so with line_remap the eight rows of a line group go to eight consecutive slots of ONE XCD, whose
    // L2 can merge the pieces into whole lines (within every run of 64 blocks: block (xcd, j) -> row 8 xcd + j).  Placement only.
    uint32_t bid = blockIdx.x;
    if (line_remap) bid = (bid & ~63u) + 8 * (bid & 7u) + ((bid >> 3) & 7u);
    const uint32_t grp = bid / rows_per_group, r = bid % rows_per_group;
    const F *in = src + (size_t)grp * src_gs + (size_t)r * src_ld;
    F *out = dst + (size_t)grp * dst_gs + (size_t)r * dst_ld;
    const uint32_t tid = threadIdx.x;
    const int plus_i = cst.w4_plus_i;
    constexpr uint32_t NLOAD = PADDED ? 2048 : 4096;
    F w[7];                                                         // the next pass's seven twiddles, requested one pass early (-2 %, same-box A/B)
#pragma unroll
    for (int t8 = 0; t8 < 7; t8++) w[t8] = ldF(tw1 + t8 * 8 + (tid & 7));          // pass 1's, in flight over the load and pass 0
#pragma unroll
    for (uint32_t i = 0; i < NLOAD; i += 512) stF(&s[fft_phys(i + tid)], ldF(in + (size_t)(i + tid) * src_es));
    __syncthreads();
    F a[8];
    {   // ---- pass 0 (h = 1): a plain 8-point DFT
        const uint32_t m = __brev(tid) >> 23;                       // rev9(b), b = tid
        a[0] = ldF(&s[fft_phys(m)]); a[2] = ldF(&s[fft_phys(m + 1024)]); a[4] = ldF(&s[fft_phys(m + 512)]); a[6] = ldF(&s[fft_phys(m + 1536)]);
        if (PADDED) { a[1] = a[0]; a[3] = a[2]; a[5] = a[4]; a[7] = a[6]; }       // (u, 0) -> (u, u)
        else {
            a[1] = ldF(&s[fft_phys(m + 2048)]); a[3] = ldF(&s[fft_phys(m + 3072)]); a[5] = ldF(&s[fft_phys(m + 2560)]); a[7] = ldF(&s[fft_phys(m + 3584)]);
            HB_DFT8_HEAD(a);
        }
        dft8_tail(a, plus_i);
        __syncthreads();                                            // every input has been read
        const uint32_t o = fft_phys(8 * tid);                       // 9*tid: positions 8b..8b+7 are contiguous
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) stF(&s[o + t8], ffold(a[t8]));
        __syncthreads();
    }
    // ---- passes 1..3: true radix-8 DIT.  Block t of the stride-h octet holds the sub-transform of the samples = rev3(t) mod 8, so
    // X[k + m h] = sum_t W_8^{rev3(t) m} (W_{8h}^{rev3(t) k} a[t]): seven general products (tables [7][h], t = 1..7), then the same
    // product-free 8-point DFT as pass 0 -- 7 instead of 12 products per octet.
#pragma unroll
    for (int pass = 1; pass <= 3; pass++) {
        const uint32_t h = pass == 1 ? 8u : pass == 2 ? 64u : 512u;
        const uint32_t k = tid & (h - 1), j = tid / h, i0 = j * 8 * h + k;
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) a[t8] = ldF(&s[fft_phys(i0 + t8 * h)]);
#pragma unroll
        for (int t8 = 1; t8 < 8; t8++) a[t8] = fmul_lz(a[t8], w[t8 - 1]);
        if (pass < 3) {                                    // next pass's twiddles: in flight over this pass's sums, stores and barrier
            const uint32_t hn = pass == 1 ? 64u : 512u;
            const F *twn = pass == 1 ? tw2 : tw3;
#pragma unroll
            for (int t8 = 0; t8 < 7; t8++) w[t8] = ldF(twn + t8 * hn + (tid & (hn - 1)));
        }
        HB_DFT8_HEAD(a);
        dft8_tail(a, plus_i);
        if (pass < 3) {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) stF(&s[fft_phys(i0 + t8 * h)], ffold(a[t8]));
            __syncthreads();
        } else {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) {
                F v = do_scale ? fmul_lz(ffold(a[t8]), scale) : fcanon(a[t8]);    // canonical out (a product already is)
                const uint32_t c = i0 + t8 * h;
                if (rot_mask)         // a commitment's rotated message half (hobbit_rot.hpp): dst_ld == 1, row r of column c at its rotated place
                    stF(out - r + msg_rot_row(r, c, rot_mask) + (size_t)c * dst_es, v);
                else
                    stF(out + (size_t)c * dst_es, v);
            }
        }
    }
}

static int launch_fft4096(hobbit_ctx *ctx, const F *src, size_t src_ld, size_t src_es, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es, const fft::R8Set &r8,
                          F scale, int do_scale, uint32_t groups, uint32_t rows_per_group, size_t src_gs, size_t dst_gs, uint32_t rot_mask = 0) {
    size_t blocks = (size_t)groups * rows_per_group;
    if (blocks == 0) return 0;
    if (rot_mask && !(src_len == 2048 && dst_ld == 1 && rot_mask == rows_per_group - 1 && (rows_per_group & rot_mask) == 0 && dst_es >= rows_per_group))
        return ctx->fail(HOBBIT_EINVAL, "fft4096: rotated stores need transposed output and a power-of-two row count");
    const size_t lds = (size_t)(4096 + 512) * 16;
    Fft4kConst cst; cst.w8 = r8.w8; cst.w8_3 = r8.w8_3; cst.w4_plus_i = r8.w4_plus_i;
    if (src_len == 2048) {
        hipFuncSetAttribute((const void *)k_fft4096<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        const int remap = (dst_ld == 1 && dst_es > 1 && rows_per_group % 64 == 0) ? 1 : 0;
        HB_LAUNCH(ctx, "k_fft4096", k_fft4096<true>, dim3((unsigned)blocks), dim3(512), lds, src, src_ld, src_es, dst, dst_ld, dst_es, r8.t1, r8.t2, r8.t3, cst,
                  scale, do_scale, rows_per_group, src_gs, dst_gs, remap, rot_mask);
    } else {
        hipFuncSetAttribute((const void *)k_fft4096<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HB_LAUNCH(ctx, "k_fft4096_full", k_fft4096<false>, dim3((unsigned)blocks), dim3(512), lds, src, src_ld, src_es, dst, dst_ld, dst_es, r8.t1, r8.t2, r8.t3,
                  cst, scale, do_scale, rows_per_group, src_gs, dst_gs, 0, 0u);
    }
    return 0;
}

// Long rows (len = R * 4096, R = 2, 4, 8; Elastic_PC opt 2 uses 32768-point row codes,
// src/Elastic_PC.cpp:737-771) by one Cooley-Tukey split:
//   X[4096 k1 + k2] = sum_{n1 < R} W_R^{n1 k1} * W_len^{n1 k2} * Y_{n1}[k2],   Y_{n1} = FFT_4096(x[R n2 + n1])
// --------------------------------------------------------------------------------------------
// The same radix-8 machinery for the shorter transforms (64 ... 2048 points): the column codes of the RS x RS tensors
// (Elastic_PC option 1: 1024 points; Our_PC option 1 and the MLP witness: 256) ran in the generic radix-2/4 kernel at log2(N)/2 products
// per element.  N = 8^P * R (R = 1, 2, 4): the R sub-sequences x[R i' + q] are transformed by P radix-8 passes (7/8 product per element
// and pass, none in the first), then ONE radix-R stage combines them (1/2 resp. 3/4 product per element): 1024 points = 2.25 N products
// instead of 5 N.  512 threads, 4096 / N rows per workgroup, the LDS layout and the lazy sums of k_fft4096.
// tabs: [pass 1 | pass 2 | ...] each [7][h] = w_N2^(rev3(t) k N2 / (8h)), then the tail [R-1][N2] = w_N^(q k).  Forward transform only.
// --------------------------------------------------------------------------------------------
template <int LOGN, bool PADDED>
__global__ void __launch_bounds__(512)
k_fft_r8(const F *__restrict__ src, size_t src_ld, F *__restrict__ dst, size_t dst_ld, size_t dst_es, const F *__restrict__ tabs, int plus_i,
         uint32_t rows_per_group, size_t src_gs, size_t dst_gs, uint32_t total_rows) {
    constexpr uint32_t N = 1u << LOGN, P = LOGN / 3, R = 1u << (LOGN % 3), N2 = N / R, TPR = N / 8, ROWS = 512 / TPR, LDR = N + N / 8, OCT = N2 / 8;
    constexpr uint32_t SRCLEN = PADDED ? N / 2 : N;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    const uint32_t tid = threadIdx.x, row0 = blockIdx.x * ROWS;
    // load: natural order, coalesced
    for (uint32_t e = tid; e < ROWS * SRCLEN; e += 512) {
        const uint32_t t = e / SRCLEN, i = e % SRCLEN, row = row0 + t;
        if (row < total_rows) {
            const F *in = src + (size_t)(row / rows_per_group) * src_gs + (size_t)(row % rows_per_group) * src_ld;
            stF(&s[t * LDR + fft_phys(i)], ldF(in + i));
        }
    }
    __syncthreads();
    const uint32_t t = tid / TPR, u = tid % TPR, q = u / OCT, b = u % OCT;
    F *sr = s + t * LDR;
    const bool live = row0 + t < total_rows;
    F a[8];
    {   // ---- pass 0 (h = 1): plain 8-point DFTs; octet b of sub-sequence q gathers x[R (rev(b) + OCT rev3(j)) + q]
        const uint32_t m = P > 1 ? (__brev(b) >> (32 - 3 * (P - 1))) : 0u;
        if (live) {
            a[0] = ldF(&sr[fft_phys(R * m + q)]); a[2] = ldF(&sr[fft_phys(R * (m + 2 * OCT) + q)]);
            a[4] = ldF(&sr[fft_phys(R * (m + OCT) + q)]); a[6] = ldF(&sr[fft_phys(R * (m + 3 * OCT) + q)]);
            if (PADDED) { a[1] = a[0]; a[3] = a[2]; a[5] = a[4]; a[7] = a[6]; }      // the upper half of the input is zero: (u, 0) -> (u, u)
            else {
                a[1] = ldF(&sr[fft_phys(R * (m + 4 * OCT) + q)]); a[3] = ldF(&sr[fft_phys(R * (m + 6 * OCT) + q)]);
                a[5] = ldF(&sr[fft_phys(R * (m + 5 * OCT) + q)]); a[7] = ldF(&sr[fft_phys(R * (m + 7 * OCT) + q)]);
                HB_DFT8_HEAD(a);
            }
            dft8_tail(a, plus_i);
        }
        __syncthreads();                                            // every input has been read
        if (live) {
            const uint32_t o = fft_phys(q * N2 + 8 * b);
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) stF(&sr[o + t8], ffold(a[t8]));
        }
        __syncthreads();
    }
    const F *tw = tabs;
#pragma unroll
    for (uint32_t pass = 1; pass < P; pass++) {
        const uint32_t h = pass == 1 ? 8u : pass == 2 ? 64u : 512u;
        const uint32_t k = b & (h - 1), j = b / h, i0 = q * N2 + j * 8 * h + k;
        if (live) {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) a[t8] = ldF(&sr[fft_phys(i0 + t8 * h)]);
#pragma unroll
            for (int t8 = 1; t8 < 8; t8++) a[t8] = fmul_lz(a[t8], ldF(tw + (t8 - 1) * h + k));
            HB_DFT8_HEAD(a);
            dft8_tail(a, plus_i);
        }
        // (an octet reads and writes the same eight slots: no barrier between its loads and stores)
        if (live) {
            if (R == 1 && pass == P - 1) {
                F *out = dst + (size_t)((row0 + t) / rows_per_group) * dst_gs + (size_t)((row0 + t) % rows_per_group) * dst_ld;
#pragma unroll
                for (int t8 = 0; t8 < 8; t8++) stF(out + (size_t)(i0 + t8 * h) * dst_es, fcanon(a[t8]));
            } else {
#pragma unroll
                for (int t8 = 0; t8 < 8; t8++) stF(&sr[fft_phys(i0 + t8 * h)], ffold(a[t8]));
            }
        }
        tw += 7 * h;
        __syncthreads();
    }
    if (R == 1 || !live) return;
    F *out = dst + (size_t)((row0 + t) / rows_per_group) * dst_gs + (size_t)((row0 + t) % rows_per_group) * dst_ld;
    if (R == 2) {               // X[k] = E[k] + w^k O[k], X[k + N/2] = E[k] - w^k O[k]
#pragma unroll
        for (uint32_t c = 0; c < N2 / TPR; c++) {
            const uint32_t k = u + TPR * c;
            const F x = ldF(&sr[fft_phys(k)]), y = fmul_lz(ldF(&sr[fft_phys(N2 + k)]), ldF(tw + k));
            stF(out + (size_t)k * dst_es, fcanon(faddl(x, y)));
            stF(out + (size_t)(k + N2) * dst_es, fcanon(fsubl<1>(x, y)));
        }
    } else {                    // X[k + m N/4] = sum_q W_4^(q m) w^(q k) S_q[k]
#pragma unroll
        for (uint32_t c = 0; c < N2 / TPR; c++) {
            const uint32_t k = u + TPR * c;
            const F y0 = ldF(&sr[fft_phys(k)]);
            const F y1 = fmul_lz(ldF(&sr[fft_phys(N2 + k)]), ldF(tw + k));
            const F y2 = fmul_lz(ldF(&sr[fft_phys(2 * N2 + k)]), ldF(tw + N2 + k));
            const F y3 = fmul_lz(ldF(&sr[fft_phys(3 * N2 + k)]), ldF(tw + 2 * N2 + k));
            const F t0 = faddl(y0, y2), t1 = fsubl<1>(y0, y2), t2 = faddl(y1, y3), t3 = fmul_w4<2>(fsubl<1>(y1, y3), plus_i);     // <= 2p + 7, 2p + 7, 2p, 2p
            stF(out + (size_t)k * dst_es, fcanon(faddl(t0, t2)));
            stF(out + (size_t)(k + N2) * dst_es, fcanon(faddl(t1, t3)));
            stF(out + (size_t)(k + 2 * N2) * dst_es, fcanon(fsubl<2>(t0, t2)));
            stF(out + (size_t)(k + 3 * N2) * dst_es, fcanon(fsubl<2>(t1, t3)));
        }
    }
}
template <int LOGN>
static int launch_fft_r8_n(hobbit_ctx *ctx, const F *src, size_t src_ld, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es, const F *tabs, int plus_i,
                           uint32_t groups, uint32_t rows_per_group, size_t src_gs, size_t dst_gs) {
    constexpr uint32_t N = 1u << LOGN, ROWS = 512 / (N / 8);
    const size_t total = (size_t)groups * rows_per_group, lds = (size_t)(4096 + 512) * 16;
    const unsigned blocks = (unsigned)((total + ROWS - 1) / ROWS);
    if (src_len == N / 2) {
        hipFuncSetAttribute((const void *)k_fft_r8<LOGN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HB_LAUNCH(ctx, "k_fft_r8", (k_fft_r8<LOGN, true>), dim3(blocks), dim3(512), lds, src, src_ld, dst, dst_ld, dst_es, tabs, plus_i, rows_per_group, src_gs, dst_gs, (uint32_t)total);
    } else {
        hipFuncSetAttribute((const void *)k_fft_r8<LOGN, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HB_LAUNCH(ctx, "k_fft_r8", (k_fft_r8<LOGN, false>), dim3(blocks), dim3(512), lds, src, src_ld, dst, dst_ld, dst_es, tabs, plus_i, rows_per_group, src_gs, dst_gs, (uint32_t)total);
    }
    return 0;
}
// src_len must be N or N/2 (zero-padded upper half); 6 <= logn <= 11
static int launch_fft_r8(hobbit_ctx *ctx, const F *src, size_t src_ld, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es, int logn, const F *tabs,
                         const fft::R8Set &r8, uint32_t groups, uint32_t rows_per_group, size_t src_gs, size_t dst_gs) {
    const int plus_i = r8.w4_plus_i;
    if ((size_t)groups * rows_per_group == 0) return 0;
    switch (logn) {
        case 6: return launch_fft_r8_n<6>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
        case 7: return launch_fft_r8_n<7>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
        case 8: return launch_fft_r8_n<8>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
        case 9: return launch_fft_r8_n<9>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
        case 10: return launch_fft_r8_n<10>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
        case 11: return launch_fft_r8_n<11>(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, tabs, plus_i, groups, rows_per_group, src_gs, dst_gs);
    }
    return ctx->fail(HOBBIT_EINVAL, "fft_r8: logn must be in [6, 11]");
}

// --------------------------------------------------------------------------------------------
// The 4096-point row code of a BASE-FIELD row (include/hobbit_real.h): 2048 reals x, zero-padded.  Two consecutive reals are the memory
// image of one F element z[j] = x[2j] + i x[2j+1], so the row is loaded as 1024 F (16 KiB) and transformed as k_fft_r8<11, true> transforms a
// zero-padded 2048-point row -- the same passes, tables and lazy sums, one row per workgroup of 256 threads, the radix-4 tail left in LDS.
// With Z = FFT_2048(z), conj(w) = 1 / w for the roots of unity of order 2^12 | p + 1 gives
//     E[k] = (Z[k] + conj(Z[-k])) / 2,   O[k] = (Z[k] - conj(Z[-k])) / (2i),   X[k] = E[k] + w^k O[k],   X[2048 - k] = conj(E[k] - w^k O[k]),
// and X[4096 - k] = conj(X[k]) makes columns 0 .. 2048 the whole row.  The unpacking pass works on the pairs (k, 2048 - k) in LDS: one product
// per pair, 1/2 = 2^60 as a one-bit rotation.  Canonical arithmetic, canonical results: the bits of k_fft4096<true> on the widened row.
// TENSOR: row (chunk chunk0 + i, r) of the launch stores X[k] into the commitment's half tensor (hobbit_half.hpp), rotated where rot_mask says so; otherwise
// row-major, 2049 elements per row.  36 KiB of LDS: four workgroups per CU.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t half61(uint64_t x) { return (x >> 1) + ((x & 1) << 60); }      // canonical x / 2: 2^60 = 1/2, and x < p keeps it below p
__device__ __forceinline__ F fhalf(const F &a) { return fmake(half61(a.re), half61(a.im)); }
template <bool TENSOR>
__global__ void __launch_bounds__(256)
k_fft_real4096(const uint64_t *__restrict__ src, F *__restrict__ dst, const F *__restrict__ tabs, const F *__restrict__ roots, int plus_i, uint32_t trs, uint32_t K,
               uint32_t rows2, uint32_t rot_mask, uint32_t chunk0, int line_remap) {
    constexpr uint32_t N = 2048, R = 4, N2 = N / R, OCT = N2 / 8, LDR = N + N / 8;
    __shared__ F s[LDR];
    // (k_fft4096's placement for transposed stores: the eight rows that share a 128-byte line of every column go to one XCD, whose L2 merges them)
    uint32_t row = blockIdx.x;
    if (line_remap) row = (row & ~63u) + 8 * (row & 7u) + ((row >> 3) & 7u);
    const uint32_t tid = threadIdx.x;
    const F *in = reinterpret_cast<const F *>(src + (size_t)row * 2048);
#pragma unroll
    for (uint32_t i = 0; i < 1024; i += 256) stF(&s[fft_phys(i + tid)], ldF(in + i + tid));
    __syncthreads();
    const uint32_t q = tid / OCT, b = tid % OCT;
    F a[8];
    {   // ---- pass 0 of k_fft_r8<11, true>: octet b of sub-sequence q gathers z[R (rev6(b) + OCT rev3(j)) + q], the upper half of the input is zero
        const uint32_t m = __brev(b) >> 26;
        a[0] = ldF(&s[fft_phys(R * m + q)]); a[2] = ldF(&s[fft_phys(R * (m + 2 * OCT) + q)]);
        a[4] = ldF(&s[fft_phys(R * (m + OCT) + q)]); a[6] = ldF(&s[fft_phys(R * (m + 3 * OCT) + q)]);
        a[1] = a[0]; a[3] = a[2]; a[5] = a[4]; a[7] = a[6];
        dft8_tail(a, plus_i);
        __syncthreads();                                            // every input has been read
        const uint32_t o = fft_phys(q * N2 + 8 * b);
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) stF(&s[o + t8], ffold(a[t8]));
        __syncthreads();
    }
    const F *tw = tabs;
#pragma unroll
    for (uint32_t pass = 1; pass < 3; pass++) {
        const uint32_t h = pass == 1 ? 8u : 64u;
        const uint32_t k = b & (h - 1), j = b / h, i0 = q * N2 + j * 8 * h + k;
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) a[t8] = ldF(&s[fft_phys(i0 + t8 * h)]);
#pragma unroll
        for (int t8 = 1; t8 < 8; t8++) a[t8] = fmul_lz(a[t8], ldF(tw + (t8 - 1) * h + k));
        HB_DFT8_HEAD(a);
        dft8_tail(a, plus_i);
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) stF(&s[fft_phys(i0 + t8 * h)], ffold(a[t8]));
        tw += 7 * h;
        __syncthreads();
    }
    // ---- the radix-4 tail, Z[k + m N/4] = sum_q W_4^(q m) w_2048^(q k) S_q[k], in place: a thread reads and writes the same four slots
#pragma unroll
    for (uint32_t c = 0; c < 2; c++) {
        const uint32_t k = tid + 256 * c;
        const F y0 = ldF(&s[fft_phys(k)]);
        const F y1 = fmul_lz(ldF(&s[fft_phys(N2 + k)]), ldF(tw + k));
        const F y2 = fmul_lz(ldF(&s[fft_phys(2 * N2 + k)]), ldF(tw + N2 + k));
        const F y3 = fmul_lz(ldF(&s[fft_phys(3 * N2 + k)]), ldF(tw + 2 * N2 + k));
        const F t0 = faddl(y0, y2), t1 = fsubl<1>(y0, y2), t2 = faddl(y1, y3), t3 = fmul_w4<2>(fsubl<1>(y1, y3), plus_i);
        stF(&s[fft_phys(k)], fcanon(faddl(t0, t2)));
        stF(&s[fft_phys(k + N2)], fcanon(faddl(t1, t3)));
        stF(&s[fft_phys(k + 2 * N2)], fcanon(fsubl<2>(t0, t2)));
        stF(&s[fft_phys(k + 3 * N2)], fcanon(fsubl<2>(t1, t3)));
    }
    __syncthreads();
    // ---- unpacking on the pairs (k, 2048 - k), k = 0 .. 1024
    const uint32_t chunk = TENSOR ? chunk0 + row / trs : 0u, r = TENSOR ? row % trs : 0u;
    auto emit = [&](uint32_t k, const F &v) {
        if (TENSOR) stF(dst + half_at(chunk, k, r, 4096u, K, rows2, rot_mask), v);
        else stF(dst + (size_t)row * 2049 + k, v);
    };
#pragma unroll
    for (uint32_t c = 0; c < 5; c++) {
        const uint32_t k = tid + 256 * c;
        if (k > 1024) break;                                        // (c == 4: thread 0 alone, the self-paired k = 1024)
        const F A = ldF(&s[fft_phys(k)]), B = fconj(ldF(&s[fft_phys((N - k) & (N - 1))]));
        const F S = fadd(A, B), D = fsub(A, B);
        const F T = fmul(fmake(D.im, D.re ? P61 - D.re : 0), ldF(roots + k));       // w^k (-i D) = 2 w^k O[k]
        emit(k, fhalf(fadd(S, T)));
        if (k != 1024) emit(N - k, fconj(fhalf(fsub(S, T))));
    }
}
// tabs: the radix-8 tables of 2048 points, roots: w^k of order 4096 (k < 2048), both forward
static int launch_fft_real4096(hobbit_ctx *ctx, const uint64_t *src, size_t rows, F *dst, const F *tabs, const F *roots, int plus_i, bool tensor, uint32_t trs,
                               uint32_t K, uint32_t rot_mask, uint32_t chunk0) {
    if (!rows) return 0;
    if (rows >> 31) return ctx->fail(HOBBIT_EINVAL, "fft_real: too many rows");
    if ((uintptr_t)src & 15) return ctx->fail(HOBBIT_EINVAL, "fft_real: the real rows must be 16-byte aligned");
    if (tensor) {
        if (!trs || rows % trs || chunk0 + rows / trs > K || (rot_mask && rot_mask != trs - 1)) return ctx->fail(HOBBIT_EINVAL, "fft_real: bad tensor shape");
        HB_LAUNCH(ctx, "k_fft_real4096", k_fft_real4096<true>, dim3((unsigned)rows), dim3(256), 0, src, dst, tabs, roots, plus_i, trs, K, 2 * trs, rot_mask, chunk0,
                  rows % 64 == 0 ? 1 : 0);
    } else
        HB_LAUNCH(ctx, "k_fft_real4096_rm", k_fft_real4096<false>, dim3((unsigned)rows), dim3(256), 0, src, dst, tabs, roots, plus_i, 0u, 0u, 0u, 0u, 0u, 0);
    return 0;
}

// The unpacking pass of k_fft_real4096 alone, for a real row code of any length L = 2 Lh (include/hobbit_elastic_real.h): Z holds, per row, the
// Lh-point transform of the row's L/2 reals read as L/4 F elements, zero-padded.  One thread per row and pair (k, Lh - k), k = 0 .. Lh / 2:
// one product with w^k (w of order L, `roots`), 1/2 as the one-bit rotation, X[k] and X[Lh - k] out; X[L - k] = conj(X[k]) is the rest.
// TENSOR: the rows are those of ONE chunk and row r stores X[k] at (r, k) of the chunk's half tensor (hobbit_half.hpp); the row index is the
// fastest thread index, so the stores of a wave are contiguous.  Otherwise row-major, Lh + 1 elements per row, k the fastest index.
template <bool TENSOR>
__global__ void __launch_bounds__(256)
k_real_unpack(const F *__restrict__ Z, F *__restrict__ dst, const F *__restrict__ roots, uint32_t Lh, uint32_t nrows, uint32_t rows2) {
    const uint32_t np = Lh / 2 + 1;
    const size_t total = (size_t)nrows * np;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = TENSOR ? (uint32_t)(g % nrows) : (uint32_t)(g / np), k = TENSOR ? (uint32_t)(g / nrows) : (uint32_t)(g % np);
        const F *z = Z + (size_t)row * Lh;
        const F A = ldF(z + k), B = fconj(ldF(z + ((Lh - k) & (Lh - 1))));
        const F S = fadd(A, B), D = fsub(A, B);
        const F T = fmul(fmake(D.im, D.re ? P61 - D.re : 0), ldF(roots + k));       // w^k (-i D) = 2 w^k O[k]
        const F lo = fhalf(fadd(S, T)), hi = fconj(fhalf(fsub(S, T)));
        if (TENSOR) {
            stF(dst + half_chunk_at(row, k, rows2), lo);
            if (2 * k != Lh) stF(dst + half_chunk_at(row, Lh - k, rows2), hi);
        } else {
            stF(dst + (size_t)row * (Lh + 1) + k, lo);
            if (2 * k != Lh) stF(dst + (size_t)row * (Lh + 1) + Lh - k, hi);
        }
    }
}
static int launch_real_unpack(hobbit_ctx *ctx, const F *Z, F *dst, const F *roots, uint32_t Lh, uint32_t nrows, bool tensor, uint32_t rows2) {
    const size_t total = (size_t)nrows * (Lh / 2 + 1);
    if (!total) return 0;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 16);
    if (tensor) HB_LAUNCH(ctx, "k_real_unpack", k_real_unpack<true>, dim3(grid), dim3(256), 0, Z, dst, roots, Lh, nrows, rows2);
    else HB_LAUNCH(ctx, "k_real_unpack_rm", k_real_unpack<false>, dim3(grid), dim3(256), 0, Z, dst, roots, Lh, nrows, 0u);
    return 0;
}
// k_real_unpack into a COMMITMENT's half tensor (hobbit_half.hpp; include/hobbit_real_rs.h): Z holds the rows of `nchunks` whole chunks of trs rows, the
// first of them chunk chunk0 of K, and row r of chunk i stores X[k] at row r of batch column half_col(i, k) -- main block and strip, where
// k_real_unpack<true> knows one chunk's block alone.  Thread index: r fastest (the stores of a wave are contiguous along the column), then the
// pair k, then the chunk, so the lines of Z a workgroup touches are those of trs adjacent rows at a few adjacent k.  Unrotated (RS x RS).
__global__ void __launch_bounds__(256)
k_real_unpack_half(const F *__restrict__ Z, F *__restrict__ dst, const F *__restrict__ roots, uint32_t Lh, uint32_t trs, uint32_t nchunks, uint32_t chunk0, uint32_t K) {
    const uint32_t np = Lh / 2 + 1, rows2 = 2 * trs, cols = 2 * Lh;
    const size_t per = (size_t)trs * np, total = per * nchunks;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t ci = (uint32_t)(g / per), e = (uint32_t)(g - (size_t)ci * per), k = e / trs, r = e - k * trs;
        const F *z = Z + ((size_t)ci * trs + r) * Lh;
        const F A = ldF(z + k), B = fconj(ldF(z + ((Lh - k) & (Lh - 1))));
        const F S = fadd(A, B), D = fsub(A, B);
        const F T = fmul(fmake(D.im, D.re ? P61 - D.re : 0), ldF(roots + k));       // w^k (-i D) = 2 w^k O[k]
        stF(dst + half_at(chunk0 + ci, k, r, cols, K, rows2, 0), fhalf(fadd(S, T)));
        if (2 * k != Lh) stF(dst + half_at(chunk0 + ci, Lh - k, r, cols, K, rows2, 0), fconj(fhalf(fsub(S, T))));
    }
}
static int launch_real_unpack_half(hobbit_ctx *ctx, const F *Z, F *dst, const F *roots, uint32_t Lh, uint32_t trs, uint32_t nchunks, uint32_t chunk0, uint32_t K) {
    const size_t total = (size_t)trs * (Lh / 2 + 1) * nchunks;
    if (!total) return 0;
    if (!trs || chunk0 + (size_t)nchunks > K) return ctx->fail(HOBBIT_EINVAL, "fft_real: bad tensor shape");
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 16);
    HB_LAUNCH(ctx, "k_real_unpack_half", k_real_unpack_half, dim3(grid), dim3(256), 0, Z, dst, roots, Lh, trs, nchunks, chunk0, K);
    return 0;
}

// The same passes for the SECOND half of a long transform (k_fft_cols's job: N-point transforms down the columns of y[n1][k2], N = len / 4096
// = 32 ... 256, inter-stage twiddle on load, result X[k1 * 4096 + k2]).  A workgroup owns C = 4096 / N adjacent columns; the column index is
// the fastest thread index, so global loads and stores are C * 16-byte runs and -- with an odd LDS row stride -- the butterflies of the 64 lanes
// of a wave fall on different banks.  Products per element: 1 (twiddle) + 7/8 per radix-8 pass after the first + 1/2 or 3/4 for the tail,
// against 1 + log2(N)/2 in the radix-2/4 stages of k_fft_cols.
// SCALE: the result leaves multiplied by `scale` (the inverse transform's 1/len; a product is canonical, so it replaces the final fold).
// WIDE: the last factor of a three-factor transform of 2^25 .. 2^28 points: the N rows are `rs` = len / N apart instead of 4096,
// a workgroup still owns C adjacent columns, and the twiddle W_len^(n1 k2), n1 k2 < 2^28, is composed from two cache-resident tables:
// tw2 = lo[b] = W^b (b < 2^14), twhi[a] = W^(a 2^14).
template <bool SCALE> __device__ __forceinline__ F fft_cols_out(const F &a, const F &scale) { return SCALE ? fmul_lz(ffold(a), scale) : fcanon(a); }
template <int LOGN, bool SCALE, bool WIDE>
__global__ void __launch_bounds__(512)
k_fft_cols_r8(const F *__restrict__ y, size_t gs, F *__restrict__ out, const F *__restrict__ tw2, const F *__restrict__ tabs, int plus_i, F scale,
              size_t rs_wide, const F *__restrict__ twhi) {
    const size_t rs = WIDE ? rs_wide : (size_t)4096;
    constexpr uint32_t N = 1u << LOGN, P = LOGN / 3, T = 1u << (LOGN % 3), N2 = N / T, TPR = N / 8, C = 4096 / N, LDR = N + N / 8 + 1, OCT = N2 / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    const uint32_t tid = threadIdx.x, k20 = blockIdx.x * C;
    const F *src = y + (size_t)blockIdx.y * gs;
    F *dst = out + (size_t)blockIdx.y * gs;
    for (uint32_t e = tid; e < C * N; e += 512) {
        const uint32_t n1 = e / C, t = e % C;
        const size_t at = (size_t)n1 * rs + k20 + t;
        F v = ldF(src + at);
        if (WIDE) {
            const uint32_t m = n1 * (k20 + t);                            // < len <= 2^28
            if (n1) v = fmul(v, fmul(ldF(twhi + (m >> 14)), ldF(tw2 + (m & 16383u))));
        } else if (n1) v = fmul(v, ldF(tw2 + at));                        // W_len^(n1 k2); row 0 of the table is all ones
        stF(&s[t * LDR + fft_phys(n1)], v);
    }
    __syncthreads();
    const uint32_t t = tid % C, u = tid / C, q = u / OCT, b = u % OCT;
    F *sr = s + t * LDR;
    F a[8];
    {   // pass 0: plain 8-point DFTs on the T interleaved sub-sequences
        const uint32_t m = P > 1 ? (__brev(b) >> (32 - 3 * (P - 1))) : 0u;
        a[0] = ldF(&sr[fft_phys(T * m + q)]); a[2] = ldF(&sr[fft_phys(T * (m + 2 * OCT) + q)]);
        a[4] = ldF(&sr[fft_phys(T * (m + OCT) + q)]); a[6] = ldF(&sr[fft_phys(T * (m + 3 * OCT) + q)]);
        a[1] = ldF(&sr[fft_phys(T * (m + 4 * OCT) + q)]); a[3] = ldF(&sr[fft_phys(T * (m + 6 * OCT) + q)]);
        a[5] = ldF(&sr[fft_phys(T * (m + 5 * OCT) + q)]); a[7] = ldF(&sr[fft_phys(T * (m + 7 * OCT) + q)]);
        HB_DFT8_HEAD(a);
        dft8_tail(a, plus_i);
        __syncthreads();
        if (P == 1 && T == 1) {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) stF(dst + (size_t)t8 * rs + k20 + t, fft_cols_out<SCALE>(a[t8], scale));
            return;
        }
        const uint32_t o = fft_phys(q * N2 + 8 * b);
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) stF(&sr[o + t8], ffold(a[t8]));
        __syncthreads();
    }
    const F *tw = tabs;
#pragma unroll
    for (uint32_t pass = 1; pass < P; pass++) {
        const uint32_t h = pass == 1 ? 8u : 64u;
        const uint32_t k = b & (h - 1), j = b / h, i0 = q * N2 + j * 8 * h + k;
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) a[t8] = ldF(&sr[fft_phys(i0 + t8 * h)]);
#pragma unroll
        for (int t8 = 1; t8 < 8; t8++) a[t8] = fmul_lz(a[t8], ldF(tw + (t8 - 1) * h + k));
        HB_DFT8_HEAD(a);
        dft8_tail(a, plus_i);
        if (T == 1 && pass == P - 1) {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) stF(dst + (size_t)(i0 + t8 * h) * rs + k20 + t, fft_cols_out<SCALE>(a[t8], scale));
        } else {
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) stF(&sr[fft_phys(i0 + t8 * h)], ffold(a[t8]));
        }
        tw += 7 * h;
        __syncthreads();
    }
    if (T == 1) return;
    if (T == 2) {
#pragma unroll
        for (uint32_t c = 0; c < N2 / TPR; c++) {
            const uint32_t k = u + TPR * c;
            const F x = ldF(&sr[fft_phys(k)]), yv = fmul_lz(ldF(&sr[fft_phys(N2 + k)]), ldF(tw + k));
            stF(dst + (size_t)k * rs + k20 + t, fft_cols_out<SCALE>(faddl(x, yv), scale));
            stF(dst + (size_t)(k + N2) * rs + k20 + t, fft_cols_out<SCALE>(fsubl<1>(x, yv), scale));
        }
    } else {
#pragma unroll
        for (uint32_t c = 0; c < N2 / TPR; c++) {
            const uint32_t k = u + TPR * c;
            const F y0 = ldF(&sr[fft_phys(k)]);
            const F y1 = fmul_lz(ldF(&sr[fft_phys(N2 + k)]), ldF(tw + k));
            const F y2 = fmul_lz(ldF(&sr[fft_phys(2 * N2 + k)]), ldF(tw + N2 + k));
            const F y3 = fmul_lz(ldF(&sr[fft_phys(3 * N2 + k)]), ldF(tw + 2 * N2 + k));
            const F t0 = faddl(y0, y2), t1 = fsubl<1>(y0, y2), t2 = faddl(y1, y3), t3 = fmul_w4<2>(fsubl<1>(y1, y3), plus_i);
            stF(dst + (size_t)k * rs + k20 + t, fft_cols_out<SCALE>(faddl(t0, t2), scale));
            stF(dst + (size_t)(k + N2) * rs + k20 + t, fft_cols_out<SCALE>(faddl(t1, t3), scale));
            stF(dst + (size_t)(k + 2 * N2) * rs + k20 + t, fft_cols_out<SCALE>(fsubl<2>(t0, t2), scale));
            stF(dst + (size_t)(k + 3 * N2) * rs + k20 + t, fft_cols_out<SCALE>(fsubl<2>(t1, t3), scale));
        }
    }
}
template <int LOGN, bool SCALE, bool WIDE>
static int launch_fft_cols_r8_n(hobbit_ctx *ctx, const F *y, size_t gs, F *out, const F *tw2, const F *tabs, int plus_i, F scale, size_t rs, const F *twhi,
                                uint32_t batch) {
    constexpr uint32_t N = 1u << LOGN, C = 4096 / N, LDR = N + N / 8 + 1;
    const size_t lds = (size_t)C * LDR * 16;
    hipFuncSetAttribute((const void *)k_fft_cols_r8<LOGN, SCALE, WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    HB_LAUNCH(ctx, WIDE ? "k_fft_cols_wide" : "k_fft_cols", (k_fft_cols_r8<LOGN, SCALE, WIDE>), dim3((unsigned)(rs / C), batch), dim3(512), lds, y, gs, out, tw2,
              tabs, plus_i, scale, rs, twhi);
    return 0;
}
template <bool SCALE>
static int launch_fft_cols_r8_s(hobbit_ctx *ctx, const F *y, size_t gs, int logr, F *out, const F *tw2, const F *tabs, int plus_i, F scale, uint32_t batch) {
    switch (logr) {
        case 5: return launch_fft_cols_r8_n<5, SCALE, false>(ctx, y, gs, out, tw2, tabs, plus_i, scale, 4096, nullptr, batch);
        case 6: return launch_fft_cols_r8_n<6, SCALE, false>(ctx, y, gs, out, tw2, tabs, plus_i, scale, 4096, nullptr, batch);
        case 7: return launch_fft_cols_r8_n<7, SCALE, false>(ctx, y, gs, out, tw2, tabs, plus_i, scale, 4096, nullptr, batch);
        case 8: return launch_fft_cols_r8_n<8, SCALE, false>(ctx, y, gs, out, tw2, tabs, plus_i, scale, 4096, nullptr, batch);
    }
    return ctx->fail(HOBBIT_EINVAL, "fft_cols_r8: R must be in [32, 256]");
}
static int launch_fft_cols_r8(hobbit_ctx *ctx, const F *y, size_t gs, int logr, F *out, const F *tw2, const F *tabs, const fft::R8Set &r8, F scale, int do_scale,
                              uint32_t batch) {
    const int plus_i = r8.w4_plus_i;
    return do_scale ? launch_fft_cols_r8_s<true>(ctx, y, gs, logr, out, tw2, tabs, plus_i, scale, batch)
                    : launch_fft_cols_r8_s<false>(ctx, y, gs, logr, out, tw2, tabs, plus_i, scale, batch);
}
// The 256-point last factor of a len = 256 * rs transform (2^25 <= len <= 2^28): y[n1][k2], rows rs apart -> X[k1 * rs + k2].  (A workgroup
// reads its 16 columns whole before it writes them and shares no address with another workgroup, so out may be y.)
static int launch_fft_cols_wide(hobbit_ctx *ctx, const F *y, size_t rs, F *out, const F *twlo, const F *twhi, const F *tabs, const fft::R8Set &r8, F scale, int do_scale) {
    const int plus_i = r8.w4_plus_i;
    if (rs < ((size_t)1 << 17) || rs > ((size_t)1 << 20) || (rs & (rs - 1))) return ctx->fail(HOBBIT_EINVAL, "fft_cols_wide: row stride must be 2^17 .. 2^20");
    if (do_scale) return launch_fft_cols_r8_n<8, true, true>(ctx, y, 0, out, twlo, tabs, plus_i, scale, rs, twhi, 1);
    return launch_fft_cols_r8_n<8, false, true>(ctx, y, 0, out, twlo, tabs, plus_i, scale, rs, twhi, 1);
}

// The R sub-transforms run in k_fft4096 (strided source); this kernel applies the twiddles and
// the R-point DFT across n1, one lane per k2 (coalesced on both sides).  tw[m] = W_len^m, m < len/2.
template <int LOGR>
__global__ void __launch_bounds__(256)
k_fft_combine(const F *__restrict__ Y, F *__restrict__ dst, size_t dst_ld, const F *__restrict__ tw, uint32_t rows) {
    constexpr uint32_t R = 1u << LOGR, len = R * 4096, half = len / 2;
    const size_t total = (size_t)rows * 4096;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(g >> 12), k2 = (uint32_t)(g & 4095);
        const F *y = Y + (size_t)row * len + k2;
        F a[R];
#pragma unroll
        for (uint32_t n1 = 0; n1 < R; n1++) {
            F v = ldF(y + (size_t)n1 * 4096);
            if (n1) {
                const uint32_t m = n1 * k2;                 // < len
                F w = ldF(tw + (m & (half - 1)));
                v = fmul(v, w);
                if (m >= half) v = fneg(v);                  // W^(m) = -W^(m - len/2)
            }
            a[__brev(n1) >> (32 - LOGR)] = v;               // bit-reversed order for the in-register DIT
        }
#pragma unroll
        for (uint32_t h = 1; h < R; h <<= 1)
#pragma unroll
            for (uint32_t b = 0; b < R / 2; b++) {
                const uint32_t k = b & (h - 1), i0 = (b / h) * 2 * h + k;
                F v = a[i0 + h];
                if (k) v = fmul(v, ldF(tw + (size_t)k * (len / (2 * h))));   // W_{2h}^k = W_len^(k len/2h)
                a[i0 + h] = fsub(a[i0], v); a[i0] = fadd(a[i0], v);
            }
        F *o = dst + (size_t)row * dst_ld + k2;
#pragma unroll
        for (uint32_t k1 = 0; k1 < R; k1++) stF(o + (size_t)k1 * 4096, a[k1]);
    }
}
static int launch_fft_combine(hobbit_ctx *ctx, int logr, const F *Y, F *dst, size_t dst_ld, const F *tw, uint32_t rows) {
    size_t total = (size_t)rows * 4096;
    if (!total) return 0;
    dim3 g(grid_for(total, 256, 1 << 16)), b(256);
    if (logr == 1) HB_LAUNCH(ctx, "k_fft_combine", k_fft_combine<1>, g, b, 0, Y, dst, dst_ld, tw, rows);
    else if (logr == 2) HB_LAUNCH(ctx, "k_fft_combine", k_fft_combine<2>, g, b, 0, Y, dst, dst_ld, tw, rows);
    else if (logr == 3) HB_LAUNCH(ctx, "k_fft_combine", k_fft_combine<3>, g, b, 0, Y, dst, dst_ld, tw, rows);
    else return ctx->fail(HOBBIT_EINVAL, "fft_combine: row length must be 8192, 16384 or 32768");
    return 0;
}

// Row-major (rows x cols) -> codeword-major (cols x ld_out) tiled transpose through LDS: both the
// global reads and the global writes are 512-byte contiguous runs.  (Writing the FFT output
// transposed directly costs a 16-byte scattered store per element: measured 22 ms vs 8 ms for the
// 2^28 commit's row pass, hence this separate, HBM-bound pass.)
__global__ void __launch_bounds__(256)
k_transpose(const F *__restrict__ in, size_t in_gs, size_t in_ld, uint32_t rows, uint32_t cols, F *__restrict__ out, size_t out_gs, size_t ld_out) {
    __shared__ F tile[32][33];
    const F *src = in + (size_t)blockIdx.z * in_gs;
    F *dst = out + (size_t)blockIdx.z * out_gs;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    const uint32_t c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t r = r0 + ty + 8 * i;
        if (r < rows && c0 + tx < cols) stF(&tile[ty + 8 * i][tx], ldF(src + (size_t)r * in_ld + c0 + tx));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t c = c0 + ty + 8 * i;
        if (c < cols && r0 + tx < rows) stF(dst + (size_t)c * ld_out + r0 + tx, ldF(&tile[tx][ty + 8 * i]));
    }
}
// Large exact multiples: 64 x 64 tiles, 1 KB contiguous on both sides instead of 512 B (measured at 2^28 on one box: 3.08 vs 3.42 ms;
// 128 x 32 and 128 x 16 tiles, longer on the write side only, gave 3.42 and 3.47).
template <int TR, int TC>
__global__ void __launch_bounds__(256)
k_transpose_big(const F *__restrict__ in, size_t in_gs, size_t in_ld, F *__restrict__ out, size_t out_gs, size_t ld_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *tile = reinterpret_cast<F *>(lds_raw);                              // [TR][TC + 1]
    const F *src = in + (size_t)blockIdx.z * in_gs;
    F *dst = out + (size_t)blockIdx.z * out_gs;
    const uint32_t c0 = blockIdx.x * TC, r0 = blockIdx.y * TR;
    {
        const uint32_t tx = threadIdx.x % TC, ty = threadIdx.x / TC;
#pragma unroll
        for (int i = 0; i < TR; i += 256 / TC) stF(&tile[(ty + i) * (TC + 1) + tx], ldF(src + (size_t)(r0 + ty + i) * in_ld + c0 + tx));
    }
    __syncthreads();
    {
        const uint32_t tx = threadIdx.x % TR, ty = threadIdx.x / TR;
#pragma unroll
        for (int i = 0; i < TC; i += 256 / TR) stF(dst + (size_t)(c0 + ty + i) * ld_out + r0 + tx, ldF(&tile[tx * (TC + 1) + ty + i]));
    }
}
int launch_transpose_ld(hobbit_ctx *ctx, const F *in, size_t in_gs, size_t in_ld, uint32_t rows, uint32_t cols, F *out, size_t out_gs, size_t ld_out,
                        uint32_t groups) {
    if (!rows || !cols || !groups) return 0;
    if (rows % 64 == 0 && cols % 64 == 0 && (size_t)rows * cols * groups >= ((size_t)1 << 24)) {
        const size_t lds = (size_t)64 * 65 * 16;
        hipFuncSetAttribute((const void *)k_transpose_big<64, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HB_LAUNCH(ctx, "k_transpose", (k_transpose_big<64, 64>), dim3(cols / 64, rows / 64, groups), dim3(256), lds, in, in_gs, in_ld, out, out_gs, ld_out);
        return 0;
    }
    HB_LAUNCH(ctx, "k_transpose", k_transpose, dim3((cols + 31) / 32, (rows + 31) / 32, groups), dim3(256), 0, in, in_gs, in_ld, rows, cols, out, out_gs,
              ld_out);
    return 0;
}
int launch_transpose(hobbit_ctx *ctx, const F *in, size_t in_gs, uint32_t rows, uint32_t cols, F *out, size_t out_gs, size_t ld_out, uint32_t groups) {
    return launch_transpose_ld(ctx, in, in_gs, cols, rows, cols, out, out_gs, ld_out, groups);
}

// Long transforms (len = 4096 * R, R up to 4096) by one Cooley-Tukey split, every pass coalesced:
//   transpose (n2,n1)->(n1,n2) | R x FFT-4096 | twiddle W_len^(n1 k2) fused into the transpose (n1,k2)->(k2,n1)
//   | 4096 x FFT-R | transpose (k2,k1)->(k1,k2).  This kernel is the middle one.  tw[m] = W_len^m, m < len/2.
// tw2 != NULL: the twiddles come from a 2-D table tw2[n1 * 4096 + k2] = W_len^(n1 k2), read with the same coalesced pattern as the data
// (the 1-D lookup tw[n1 k2 mod half] is a 16-byte load per lane from 64 different cache lines: 0.71 -> see DESIGN.md 4).
__global__ void __launch_bounds__(256)
k_transpose_tw(const F *__restrict__ in, size_t gs, uint32_t R, F *__restrict__ out, const F *__restrict__ tw, uint32_t half, const F *__restrict__ tw2) {
    __shared__ F tile[32][33];
    const F *src = in + (size_t)blockIdx.z * gs;
    F *dst = out + (size_t)blockIdx.z * gs;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t k20 = blockIdx.x * 32, n10 = blockIdx.y * 32;          // input: R rows (n1) x 4096 cols (k2)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t n1 = n10 + ty + 8 * i, k2 = k20 + tx;
        if (n1 < R) {
            F v = ldF(src + (size_t)n1 * 4096 + k2);
            const uint32_t m = n1 * k2;                                   // < len = 2*half
            if (tw2) { if (m) v = fmul(v, ldF(tw2 + (size_t)n1 * 4096 + k2)); }
            else if (m) { v = fmul(v, ldF(tw + (m & (half - 1)))); if (m >= half) v = fneg(v); }
            stF(&tile[ty + 8 * i][tx], v);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t k2 = k20 + ty + 8 * i, n1 = n10 + tx;
        if (n1 < R) stF(dst + (size_t)k2 * R + n1, ldF(&tile[tx][ty + 8 * i]));
    }
}
__global__ void __launch_bounds__(256)
k_build_tw2d(const F *__restrict__ tw, uint32_t half, uint32_t R, F *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)R * 4096) return;
    const uint32_t n1 = (uint32_t)(i >> 12), k2 = (uint32_t)(i & 4095), m = n1 * k2;
    F v = ldF(tw + (m & (half - 1)));
    if (m >= half) v = fneg(v);
    stF(out + i, v);
}
static int launch_build_tw2d(hobbit_ctx *ctx, const F *tw, uint32_t half, uint32_t R, F *out) {
    HB_LAUNCH(ctx, "k_build_tw2d", k_build_tw2d, dim3((unsigned)(((size_t)R * 4096 + 255) / 256)), dim3(256), 0, tw, half, R, out);
    return 0;
}
static int launch_transpose_tw(hobbit_ctx *ctx, const F *in, size_t gs, uint32_t R, F *out, const F *tw, uint32_t half, const F *tw2, uint32_t groups) {
    HB_LAUNCH(ctx, "k_transpose_tw", k_transpose_tw, dim3(4096 / 32, (R + 31) / 32, groups), dim3(256), 0, in, gs, R, out, tw, half, tw2);
    return 0;
}

namespace fft {

// ---- tables: each built on first use per context, uploaded synchronously, and the context's until it goes (ctx->helper / helper2: their own)
static int table(hobbit_ctx *ctx, Kind kind, int logn, bool inverse, const F **out) {
    auto &dev = ctx->fft.dev;
    const auto key = std::make_tuple((int)kind, logn, inverse);
    auto it = dev.find(key);
    if (it == dev.end()) {
        mem::Buf<F> d;
        if (kind == TW2D) {
            const F *tw; HB_TRY(table(ctx, ROOTS, logn, inverse, &tw));
            if (d.alloc((size_t)1 << logn)) return ctx->fail(HOBBIT_ENOMEM, "twiddle table alloc failed");
            HB_TRY(launch_build_tw2d(ctx, tw, 1u << (logn - 1), 1u << (logn - 12), d));
        } else {
            const std::vector<F> t = build_table(kind, logn, inverse);
            if (d.alloc(t.size())) return ctx->fail(HOBBIT_ENOMEM, "twiddle alloc failed");
            HB_CHECK(ctx, hipMemcpy(d, t.data(), t.size() * sizeof(F), hipMemcpyHostToDevice));
        }
        it = dev.emplace(key, std::move(d)).first;
    }
    *out = it->second;
    return 0;
}
int roots(hobbit_ctx *ctx, int logn, bool inverse, const F **out) { return table(ctx, ROOTS, logn, inverse, out); }
static int r8_set(hobbit_ctx *ctx, bool inverse, const R8Set **out) {
    R8Set &r = ctx->fft.r8[inverse ? 1 : 0];
    if (!r.t1) {
        const R8Roots c = r8_roots(inverse);
        if (c.w4.re != 0 || (c.w4.im != 1 && c.w4.im != P61 - 1)) return ctx->fail(HOBBIT_EINVAL, "unexpected 4th root of unity");
        const F *t; HB_TRY(table(ctx, RADIX8, 12, inverse, &t));
        r.t2 = t + 7 * 8; r.t3 = t + 7 * 8 + 7 * 64; r.w8 = c.w8; r.w8_3 = c.w8_3; r.w4_plus_i = c.w4.im == 1; r.t1 = t;
    }
    *out = &r;
    return 0;
}
static Scale resolve(Scale s, int logn, bool inverse) {
    if (s.on < 0) { s.on = inverse ? 1 : 0; if (inverse) s.by = finv(fmake((uint64_t)1 << logn)); }
    return s;
}

// ---- dispatch: the 4096-point kernel and the radix-8 kernels where they apply, the generic LDS kernel otherwise
int rows(hobbit_ctx *ctx, const F *src, size_t src_ld, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es, int logn, bool inverse, uint32_t groups,
         uint32_t rows_per_group, size_t src_gs, size_t dst_gs, Scale out) {
    out = resolve(out, logn, inverse);
    const R8Set *r8;
    if (logn == 12 && (src_len == 2048 || src_len == 4096)) {
        HB_TRY(r8_set(ctx, inverse, &r8));
        return launch_fft4096(ctx, src, src_ld, 1, src_len, dst, dst_ld, dst_es, *r8, out.by, out.on, groups, rows_per_group, src_gs, dst_gs);
    }
    if (!inverse && logn >= 6 && logn <= 11 && (src_len == (1u << logn) || src_len == (1u << (logn - 1)))) {
        HB_TRY(r8_set(ctx, false, &r8));
        const F *tabs; HB_TRY(table(ctx, RADIX8, logn, false, &tabs));
        return launch_fft_r8(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, logn, tabs, *r8, groups, rows_per_group, src_gs, dst_gs);
    }
    const F *tw; HB_TRY(roots(ctx, logn, inverse, &tw));
    return launch_fft_rows(ctx, src, src_ld, src_len, dst, dst_ld, dst_es, logn, tw, out.by, out.on, groups, rows_per_group, src_gs, dst_gs);
}
int rowcode_4096(hobbit_ctx *ctx, const F *src, size_t src_ld, F *dst, size_t dst_ld, size_t dst_es, uint32_t groups, uint32_t rows_per_group, size_t src_gs,
                 size_t dst_gs, uint32_t rot_mask) {
    const R8Set *r8; HB_TRY(r8_set(ctx, false, &r8));
    return launch_fft4096(ctx, src, src_ld, 1, 2048, dst, dst_ld, dst_es, *r8, fmake(1), 0, groups, rows_per_group, src_gs, dst_gs, rot_mask);
}
int rowcode_real4096(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, F *dst, bool tensor, uint32_t trs, uint32_t K, uint32_t rot_mask, uint32_t chunk0) {
    const R8Set *r8; HB_TRY(r8_set(ctx, false, &r8));
    const F *tabs, *tw; HB_TRY(table(ctx, RADIX8, 11, false, &tabs)); HB_TRY(roots(ctx, 12, false, &tw));
    return launch_fft_real4096(ctx, src, nrows, dst, tabs, tw, r8->w4_plus_i, tensor, trs, K, rot_mask, chunk0);
}
int rowcode_combine(hobbit_ctx *ctx, const F *msg, int logc, uint32_t nrows, F *Y, F *rm) {
    const int lr = logc - 12; const uint32_t R = 1u << lr; const size_t cols = (size_t)1 << logc;
    const R8Set *r8; HB_TRY(r8_set(ctx, false, &r8));
    HB_TRY(launch_fft4096(ctx, msg, 1, R, 2048, Y, 4096, 1, *r8, fmake(1), 0, nrows, R, cols / 2, cols));
    const F *twl; HB_TRY(roots(ctx, logc, false, &twl));
    return launch_fft_combine(ctx, lr, Y, rm, cols, twl, nrows);
}

// Long forward/inverse transform of `batch` rows: row b of src (src_len nonzero elements, the rest of the 2^logn
// transform length zero) -> row b of dst (2^logn elements, contiguous).  13 <= logn <= 24.  src may equal dst.
// `out` is fused into the last arithmetic pass (a nested call of a longer transform passes none).  An inverse transform takes full-length sources only.
static int long_rows(hobbit_ctx *ctx, const F *src, size_t src_ld, size_t src_len, F *dst, int logn, bool inverse, uint32_t batch, Scale out = Scale()) {
    const size_t len = (size_t)1 << logn; const int lr = logn - 12; const uint32_t R = 1u << lr;
    if (lr < 1 || lr > 12) return ctx->fail(HOBBIT_EINVAL, "fft_long: the two-factor form serves logn in [13,24]");
    if (src_len != len && (inverse || src_len != len / 2)) return ctx->fail(HOBBIT_EINVAL, "fft_long: source must be the full length or, forward, its zero-padded half");
    if ((size_t)batch * 4096 >> 32) return ctx->fail(HOBBIT_EINVAL, "fft_long: too many rows");
    out = resolve(out, logn, inverse);
    F *t1, *t2;
    HB_TRY(ctx->workspace((size_t)batch * len * sizeof(F), (void **)&t1));
    HB_TRY(ctx->workspace2((size_t)batch * len * sizeof(F), (void **)&t2));
    const F *twl; HB_TRY(roots(ctx, logn, inverse, &twl));
    const R8Set *r8; HB_TRY(r8_set(ctx, inverse, &r8));
    const uint32_t sub_len = src_len == len ? 4096u : 2048u;
    if (R <= 64) {
        // short strides: the R sub-transforms read x[R n2 + n1] in place (element stride R) -- adjacent n1 share cache lines, and the
        // separate transpose pass costs more than it saves (measured: -0.15 ms per shockwave_prove; for R >= 128 the transpose wins)
        HB_TRY(launch_fft4096(ctx, src, 1, R, sub_len, t1, 4096, 1, *r8, fmake(1), 0, batch, R, src_ld, len));
    } else {
        // (n2, n1) -> (n1, n2); only the nonzero n2 rows are moved (x[R n2 + n1] != 0 needs n2 < src_len / R)
        HB_TRY(launch_transpose_ld(ctx, src, src_ld, R, (uint32_t)(src_len / R), R, t1, len, 4096, batch));
        HB_TRY(launch_fft4096(ctx, t1, 4096, 1, sub_len, t1, 4096, 1, *r8, fmake(1), 0, batch, R, len, len));
    }
    // inter-stage twiddles as a 2-D table (len entries, built once per length and direction, <= 32 MB)
    const F *tw2 = nullptr;
    if (logn <= 21) HB_TRY(table(ctx, TW2D, logn, inverse, &tw2));
    if (tw2 && lr >= 2 && lr <= 8 && batch <= 65535) {
        // one pass: twiddle on load, 16 columns x R rows per workgroup, final order on store (t1 -> dst; src was consumed above)
        if (lr >= 5) {
            const F *tabs; HB_TRY(table(ctx, RADIX8, lr, inverse, &tabs));
            return launch_fft_cols_r8(ctx, t1, len, lr, dst, tw2, tabs, *r8, out.by, out.on, batch);
        }
        const F *twr; HB_TRY(roots(ctx, lr, inverse, &twr));
        return launch_fft_cols(ctx, t1, len, lr, dst, tw2, twr, out.by, out.on, batch);
    }
    HB_TRY(launch_transpose_tw(ctx, t1, len, R, t2, twl, (uint32_t)(len / 2), tw2, batch));
    // (forward, the R-point rows run as before: radix-8 where it is built; the inverse's 1/len rides on this pass, the last with arithmetic)
    HB_TRY(rows(ctx, t2, R, R, t2, R, 1, lr, inverse, 1, (uint32_t)((size_t)batch * 4096), 0, 0, out));
    return launch_transpose_ld(ctx, t2, len, R, 4096, R, dst, len, 4096, batch);
}

// 2^25 <= len <= 2^28 as three factors, len = 256 * S = 256 * (4096 * R'), in place on `batch` contiguous rows (one row at a time: a row alone
// fills the chip).  x[256 m + n1] is moved to y[n1][m] (workspace5), the 256 rows of S = 2^17 .. 2^20 points are transformed by the two-factor
// form above (one batched call, workspace / workspace2), and the 256-point last factor takes its twiddle W_len^(n1 k2) from the split tables and
// writes X[k1 S + k2] back over the input.  Sweeps over the data: transpose, (transpose for S >= 2^19,) FFT-4096, S-columns, 256-columns = 4 or 5.
static int wide_rows(hobbit_ctx *ctx, F *data, int logn, bool inverse, size_t batch) {
    if (logn < 25 || logn > 28) return ctx->fail(HOBBIT_EINVAL, "fft_wide: the three-factor form serves logn in [25,28]");
    const size_t len = (size_t)1 << logn, S = len >> 8;
    F *y; HB_TRY(ctx->workspace5(len * sizeof(F), (void **)&y));
    const F *lo; HB_TRY(table(ctx, SPLIT, logn, inverse, &lo));
    const F *tabs; HB_TRY(table(ctx, RADIX8, 8, inverse, &tabs));
    const R8Set *r8; HB_TRY(r8_set(ctx, inverse, &r8));
    const Scale out = resolve(Scale(), logn, inverse);
    for (size_t b = 0; b < batch; b++) {
        F *x = data + b * len;
        HB_TRY(launch_transpose_ld(ctx, x, 0, 256, (uint32_t)S, 256, y, 0, S, 1));
        HB_TRY(long_rows(ctx, y, S, S, y, logn - 8, inverse, 256, Scale::none()));
        HB_TRY(launch_fft_cols_wide(ctx, y, S, x, lo, lo + SPLIT_LO, tabs, *r8, out.by, out.on));
    }
    return 0;
}
int any_rows(hobbit_ctx *ctx, const F *src, size_t src_ld, size_t src_len, F *dst, int logn, bool inverse, size_t batch) {
    const size_t len = (size_t)1 << logn;
    if (logn <= 12) return rows(ctx, src, src_ld, (uint32_t)src_len, dst, len, 1, logn, inverse, 1, (uint32_t)batch, 0, 0);
    if (logn <= 24) return long_rows(ctx, src, src_ld, src_len, dst, logn, inverse, (uint32_t)batch);
    if (src == dst && (src_len != len || src_ld != len)) return ctx->fail(HOBBIT_EINVAL, "fft: in place, rows of 2^25 and more must be full and contiguous");
    if (src != dst) {
        for (size_t b = 0; b < batch; b++) {
            HB_TRY(launch_copy(ctx, dst + b * len, src + b * src_ld, src_len * sizeof(F)));
            if (src_len < len) HB_TRY(launch_zero(ctx, dst + b * len + src_len, (len - src_len) * sizeof(F)));
        }
    }
    return wide_rows(ctx, dst, logn, inverse, batch);
}

// the packed transform of `nrows` real rows of Lh reals: row r is Lh / 2 F elements, zero-padded to Lh points, into workspace5 (the long transform owns
// workspace / workspace2)
static int real_packed(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F **Z) {
    const size_t Lh = (size_t)1 << (logL - 1);
    HB_TRY(ctx->workspace5(nrows * Lh * sizeof(F), (void **)Z));
    return any_rows(ctx, reinterpret_cast<const F *>(src), Lh / 2, Lh / 2, *Z, logL - 1, false, nrows);
}
static int real_rows_impl(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst, bool tensor, uint32_t trs);
int real_rows_any(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst, bool tensor, uint32_t trs) {
    if (logL < 3 || logL > 16) return ctx->fail(HOBBIT_EINVAL, "fft_real_rows_any: logL must be in [3,16]");
    return real_rows_impl(ctx, src, nrows, logL, dst, tensor, trs);
}
int real_rows_len(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst) {
    if (logL < 3 || logL > 20) return ctx->fail(HOBBIT_EINVAL, "fft_real_rows_len: logL must be in [3,20]");
    return real_rows_impl(ctx, src, nrows, logL, dst, false, 0);
}
int rowcode_real_half(hobbit_ctx *ctx, const uint64_t *src, int logL, F *dst, uint32_t trs, uint32_t K, uint32_t nchunks, uint32_t chunk0) {
    if (logL < 3 || logL > 20) return ctx->fail(HOBBIT_EINVAL, "fft_real: the row code of a half commitment has 2^3 .. 2^20 points");
    if (!trs || !nchunks || chunk0 + (size_t)nchunks > K) return ctx->fail(HOBBIT_EINVAL, "fft_real: bad tensor shape");
    const size_t nrows = (size_t)nchunks * trs;
    if (logL == 12) return rowcode_real4096(ctx, src, nrows, dst, true, trs, K, 0, chunk0);
    if ((uintptr_t)src & 15) return ctx->fail(HOBBIT_EINVAL, "fft_real: the real rows must be 16-byte aligned");
    F *Z; HB_TRY(real_packed(ctx, src, nrows, logL, &Z));
    const F *tw; HB_TRY(roots(ctx, logL, false, &tw));
    return launch_real_unpack_half(ctx, Z, dst, tw, 1u << (logL - 1), trs, nchunks, chunk0, K);
}
static int real_rows_impl(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst, bool tensor, uint32_t trs) {
    if (!nrows) return 0;
    if (nrows >> 20) return ctx->fail(HOBBIT_EINVAL, "fft_real: too many rows");
    if (tensor && (!trs || nrows != trs)) return ctx->fail(HOBBIT_EINVAL, "fft_real: the tensor form takes the rows of one chunk");
    if (logL == 12) return rowcode_real4096(ctx, src, nrows, dst, tensor, trs, 1, 0, 0);
    if ((uintptr_t)src & 15) return ctx->fail(HOBBIT_EINVAL, "fft_real: the real rows must be 16-byte aligned");
    const size_t Lh = (size_t)1 << (logL - 1);
    F *Z; HB_TRY(real_packed(ctx, src, nrows, logL, &Z));
    const F *tw; HB_TRY(roots(ctx, logL, false, &tw));
    return launch_real_unpack(ctx, Z, dst, tw, (uint32_t)Lh, (uint32_t)nrows, tensor, 2 * trs);
}

}  // namespace fft
}  // namespace hobbit

using namespace hobbit;

extern "C" {

int hobbit_fft_batch(hobbit_ctx *ctx, hobbit_F *d_data, int logn, size_t batch, size_t ld, int inverse) {
    if (logn < 0 || logn > 24) return ctx->fail(HOBBIT_EINVAL, "fft_batch: logn must be in [0,24]");
    if (logn == 0 || batch == 0) return 0;
    if (ld < ((size_t)1 << logn)) return ctx->fail(HOBBIT_EINVAL, "fft_batch: ld < 2^logn");
    F *d = reinterpret_cast<F *>(d_data);
    if (logn > 12) {
        if (inverse) return ctx->fail(HOBBIT_EINVAL, "fft_batch: inverse transforms longer than 4096 are not built (the hot path only needs forward)");
        if (ld != ((size_t)1 << logn)) return ctx->fail(HOBBIT_EINVAL, "fft_batch: long rows must be contiguous");
        return fft::any_rows(ctx, d, ld, ld, d, logn, false, (uint32_t)batch);
    }
    return fft::rows(ctx, d, ld, 1u << logn, d, ld, 1, logn, inverse != 0, 1, (uint32_t)batch, 0, 0);
}
int hobbit_fft_real_rows(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, hobbit_F *d_out) {
    if (!rows) return 0;
    if (!d_reals || !d_out) return ctx->fail(HOBBIT_EINVAL, "fft_real_rows: null argument");
    return fft::rowcode_real4096(ctx, d_reals, rows, reinterpret_cast<F *>(d_out), false, 0, 0, 0, 0);
}
int hobbit_fft_real_rows_any(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, int logL, hobbit_F *d_out) {
    if (rows && (!d_reals || !d_out)) return ctx->fail(HOBBIT_EINVAL, "fft_real_rows_any: null argument");
    return fft::real_rows_any(ctx, d_reals, rows, logL, reinterpret_cast<F *>(d_out), false, 0);
}
int hobbit_fft_real_rows_len(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, int logL, hobbit_F *d_out) {
    if (rows && (!d_reals || !d_out)) return ctx->fail(HOBBIT_EINVAL, "fft_real_rows_len: null argument");
    return fft::real_rows_len(ctx, d_reals, rows, logL, reinterpret_cast<F *>(d_out));
}
int hobbit_fft_any(hobbit_ctx *ctx, hobbit_F *d_data, int logn, size_t batch, size_t ld, int inverse) {
    if (logn < 1 || logn > 28) return ctx->fail(HOBBIT_EINVAL, "fft_any: logn must be in [1,28]");
    const size_t len = (size_t)1 << logn;
    if (!d_data) return ctx->fail(HOBBIT_EINVAL, "fft_any: null data");
    if (batch > (((size_t)1 << 30) >> logn)) return ctx->fail(HOBBIT_EINVAL, "fft_any: batch * 2^logn must not exceed 2^30");
    if (ld < len) return ctx->fail(HOBBIT_EINVAL, "fft_any: ld < 2^logn");
    if (logn > 12 && ld != len) return ctx->fail(HOBBIT_EINVAL, "fft_any: rows longer than 4096 must be contiguous");
    if (batch == 0) return 0;
    F *d = reinterpret_cast<F *>(d_data);
    if (logn <= 12) return fft::rows(ctx, d, ld, (uint32_t)len, d, ld, 1, logn, inverse != 0, 1, (uint32_t)batch, 0, 0);
    return fft::any_rows(ctx, d, len, len, d, logn, inverse != 0, batch);
}

}  // extern "C"
