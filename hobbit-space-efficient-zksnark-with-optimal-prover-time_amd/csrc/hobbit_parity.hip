// hobbit_parity.hip -- the C ABI of include/hobbit_parity.h: commit_parity_matrix, open_parity_matrix and prove_linear_code_batch
// (src/sumcheck.cpp:2622-2885, 3201-3221).  The sub-provers (multiplication tree, sumchecks, shockwave commit / prove, eq tables) are the
// library's own entry points; this file adds what lies between them: the access lists (public data of the graphs: on the host in
// hobbit_parity_commit, by kernels in hobbit_parity_commit_device of include/hobbit_parity_lists.h), and the kernels that turn lists and
// challenges into the provers' inputs.  No list goes back to the host during an opening.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include "hobbit_kernels.hpp"
#include "hobbit_libcgen.hpp"
#include "../../include/hobbit_parity.h"
#include "../../include/hobbit_parity_lists.h"

using namespace hobbit;

static inline CHP cF(const hobbit_F *p) { return CHP(reinterpret_cast<const HF *>(p)); }
static inline MHP mF(hobbit_F *p) { return MHP(reinterpret_cast<HF *>(p)); }
static inline hobbit_F *aF(F *p) { return reinterpret_cast<hobbit_F *>(p); }
static inline const hobbit_F *aF(const F *p) { return reinterpret_cast<const hobbit_F *>(p); }

namespace {

constexpr int PB = 256;                       // threads per workgroup of every kernel here
static inline uint32_t pgrid(size_t n, uint32_t cap = 1u << 16) { size_t g = (n + PB - 1) / PB; return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g); }

// ---- the fused gather: one pass over the P list entries ---------------------------------------------------------------------------------------
// betas1[i] = eq(r1)[idx1[i]], betas2[i] = eq(r2)[idx2[i]] (zero for m <= i < P, where idx = cnt = 0 too) and the four rows of the first
// multiplication tree (src/sumcheck.cpp:2756-2763):  rows 0 / 2: a idx + b (cnt - 1) + beta + 1,  rows 1 / 3: a idx + b cnt + beta + 1.
// The two tables have 2n entries of 16 bytes: L2-resident up to about n = 2^17, so the random reads cost no HBM traffic there; the lists are
// read and the six outputs written once, coalesced.
__global__ void __launch_bounds__(PB) k_parity_gather(const uint32_t *__restrict__ idx1, const uint32_t *__restrict__ idx2, const uint32_t *__restrict__ cnt1,
                                                      const uint32_t *__restrict__ cnt2, const F *__restrict__ beta1, const F *__restrict__ beta2, F a, F b, size_t m,
                                                      size_t P, F *__restrict__ betas12, F *__restrict__ rows) {
    const F one = fmake(1), zero = fmake(0);
    for (size_t i = blockIdx.x * (size_t)PB + threadIdx.x; i < P; i += (size_t)gridDim.x * PB) {
        const uint32_t i1 = idx1[i], i2 = idx2[i], c1 = cnt1[i], c2 = cnt2[i];
        const F b1 = i < m ? beta1[i1] : zero, b2 = i < m ? beta2[i2] : zero;
        betas12[i] = b1; betas12[P + i] = b2;
        const F t1 = fadd(fadd(fmul32(a, i1), fmul32(b, c1)), fadd(b1, one)), t2 = fadd(fadd(fmul32(a, i2), fmul32(b, c2)), fadd(b2, one));
        rows[i] = fsub(t1, b); rows[P + i] = t1; rows[2 * P + i] = fsub(t2, b); rows[3 * P + i] = t2;
    }
}

// ---- the fused evaluation: <eq, idx1>, <eq, idx2>, <eq, cnt1>, <eq, cnt2>, <eq, weight>, <eq, betas1>, <eq, betas2> over i < m (:2772-2780) ----
// A thread keeps its seven sums unreduced (128-bit per component: canonical products below 2^61, at most 2^25 of them) and folds once.
struct Acc { u128 re, im; };
__device__ __forceinline__ void acc_add(Acc &s, const F &v) { s.re += v.re; s.im += v.im; }
__device__ __forceinline__ F acc_fold(const Acc &s) { return fmake(red124(s.re), red124(s.im)); }
template <int K>
__device__ __forceinline__ void block_sum_store(F *v, F *__restrict__ out) {      // out[k] = sum over the workgroup of v[k]
    __shared__ F sh[K][PB];
    for (int k = 0; k < K; k++) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int s = PB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) for (int k = 0; k < K; k++) sh[k][threadIdx.x] = fadd(sh[k][threadIdx.x], sh[k][threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < K) out[threadIdx.x] = sh[threadIdx.x][0];
}
__global__ void __launch_bounds__(PB) k_parity_eval(const F *__restrict__ eq, const uint32_t *__restrict__ idx1, const uint32_t *__restrict__ idx2,
                                                    const uint32_t *__restrict__ cnt1, const uint32_t *__restrict__ cnt2, const F *__restrict__ weight,
                                                    const F *__restrict__ betas12, size_t m, size_t P, F *__restrict__ partials) {
    Acc s[7];
    for (int k = 0; k < 7; k++) { s[k].re = 0; s[k].im = 0; }
    for (size_t i = blockIdx.x * (size_t)PB + threadIdx.x; i < m; i += (size_t)gridDim.x * PB) {
        const F e = eq[i];
        acc_add(s[0], fmul32(e, idx1[i])); acc_add(s[1], fmul32(e, idx2[i])); acc_add(s[2], fmul32(e, cnt1[i])); acc_add(s[3], fmul32(e, cnt2[i]));
        acc_add(s[4], fmul(e, weight[i])); acc_add(s[5], fmul(e, betas12[i])); acc_add(s[6], fmul(e, betas12[P + i]));
    }
    F v[7];
    for (int k = 0; k < 7; k++) v[k] = acc_fold(s[k]);
    block_sum_store<7>(v, partials + 7 * (size_t)blockIdx.x);
}
__global__ void __launch_bounds__(PB) k_parity_eval_final(const F *__restrict__ partials, uint32_t nb, F *__restrict__ out) {
    F v[7];
    for (int k = 0; k < 7; k++) v[k] = fmake(0);
    for (uint32_t j = threadIdx.x; j < nb; j += PB) for (int k = 0; k < 7; k++) v[k] = fadd(v[k], partials[7 * (size_t)j + k]);
    block_sum_store<7>(v, out);
}

// ---- input rows of the second tree over the S = 2n cells (:2788-2795): a i + beta + 1 and b accesses + a i + beta + 1 ----------------------------
__global__ void __launch_bounds__(PB) k_parity_tree2(const F *__restrict__ beta1, const F *__restrict__ beta2, const F *__restrict__ acc1, const F *__restrict__ acc2,
                                                     F a, F b, size_t S, F *__restrict__ rows) {
    const F one = fmake(1);
    for (size_t i = blockIdx.x * (size_t)PB + threadIdx.x; i < S; i += (size_t)gridDim.x * PB) {
        const F ai = fmul32(a, (uint32_t)i);
        const F u1 = fadd(fadd(ai, beta1[i]), one), u2 = fadd(fadd(ai, beta2[i]), one);
        rows[i] = u1; rows[S + i] = fadd(fmul(b, acc1[i]), u1); rows[2 * S + i] = u2; rows[3 * S + i] = fadd(fmul(b, acc2[i]), u2);
    }
}

// ---- the public witness, 8P F (:2692-2704 and :2846-2858): idx1 at 0, idx2 at off2 (m in the commit, P in the open), cnt1 at 2P, cnt2 at 3P,
// weight at 4P, acc1 at 5P, acc2 at 5P + S, zeros elsewhere
__global__ void __launch_bounds__(PB) k_parity_witness(const uint32_t *__restrict__ idx1, const uint32_t *__restrict__ idx2, const uint32_t *__restrict__ cnt1,
                                                       const uint32_t *__restrict__ cnt2, const F *__restrict__ weight, const F *__restrict__ acc1,
                                                       const F *__restrict__ acc2, size_t m, size_t P, size_t off2, size_t S, F *__restrict__ out) {
    for (size_t i = blockIdx.x * (size_t)PB + threadIdx.x; i < 8 * P; i += (size_t)gridDim.x * PB) {
        F v = fmake(0);
        if (i < 2 * P) {
            if (i < m) v = fmake(idx1[i]);
            else if (i >= off2 && i < off2 + m) v = fmake(idx2[i - off2]);
        } else if (i < 3 * P) v = fmake(cnt1[i - 2 * P]);
        else if (i < 4 * P) v = fmake(cnt2[i - 3 * P]);
        else if (i < 5 * P) v = weight[i - 4 * P];
        else if (i < 5 * P + S) v = acc1[i - 5 * P];
        else if (i < 5 * P + 2 * S) v = acc2[i - 5 * P - S];
        out[i] = v;
    }
}

// ---- prove_linear_code_batch's row combination (:3208-3212): B[j] = sum_i eq(r2)[i] codeword_i[j], zero past a codeword's end ---------------------
__global__ void __launch_bounds__(PB) k_parity_batch_rows(const F *__restrict__ cw, size_t count, size_t ld, size_t len, const F *__restrict__ beta2, size_t S,
                                                          F *__restrict__ B) {
    for (size_t j = blockIdx.x * (size_t)PB + threadIdx.x; j < S; j += (size_t)gridDim.x * PB) {
        F s = fmake(0);
        if (j < len) for (size_t i = 0; i < count; i++) s = fadd(s, fmul(beta2[i], cw[i * ld + j]));
        B[j] = s;
    }
}

// ---- the access lists built on the device (hobbit_parity_commit_device) -------------------------------------------------------------------------
// The lists are a function of the code's forward form and its segment table (hobbit_ctx.hpp ParitySeg; hobbit_capi.hip ensure_fwd).  One fill
// pass writes idx1, idx2, weight and cnt2; cnt1 -- the rank of an entry among the entries of the same idx1 cell, in list order -- comes from
// one stable sort of the m positions by cell (rocprim's radix sort over log2 2n key bits): the sorted run of a cell lists its entries in list
// order whatever the graphs' in-degrees are, so the rank is the place in the run and the run's length is the cell's access count.
constexpr uint32_t MAX_SEGS = 400;            // four per depth; hobbit_graph_upload takes depths below 100

// occurrences of the idx2 cell c in segments [0, upto): a segment covers an interval of cells, each `degree` times
__device__ __forceinline__ uint32_t cell_count2(const ParitySeg *sg, uint32_t upto, uint32_t c) {
    uint32_t k = 0;
    for (uint32_t s = 0; s < upto; s++) if (c - sg[s].off < sg[s].cells) k += sg[s].degree;
    return k;
}
// Four consecutive entries per lane: the three u32 lists go out 16 B per lane, the weights 64 B per lane.  Entries from m on are zero.
__global__ void __launch_bounds__(PB) k_parity_fill(const ParitySeg *__restrict__ segs, uint32_t nseg, const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ w32,
                                                    const F *__restrict__ wF, size_t m, size_t P, uint32_t *__restrict__ idx1, uint32_t *__restrict__ idx2,
                                                    uint32_t *__restrict__ cnt2, F *__restrict__ weight) {
    __shared__ ParitySeg sg[MAX_SEGS];
    for (uint32_t i = threadIdx.x; i < nseg; i += PB) sg[i] = segs[i];
    __syncthreads();
    const F minus1 = fmake(P61 - 1), zero = fmake(0);
    for (size_t q = blockIdx.x * (size_t)PB + threadIdx.x; q < P / 4; q += (size_t)gridDim.x * PB) {
        const size_t e0 = 4 * q;
        uint32_t s = 0, hi = nseg;                                   // the last segment that starts at or before e0
        while (hi - s > 1) { const uint32_t mid = (s + hi) / 2; if (sg[mid].base <= e0) s = mid; else hi = mid; }
        uint32_t a[4], b[4], c2[4]; F w[4];
        for (int k = 0; k < 4; k++) {
            const size_t e = e0 + k;
            a[k] = b[k] = c2[k] = 0; w[k] = zero;
            if (e >= m) continue;
            while (e - sg[s].base >= sg[s].count) s++;
            const uint32_t j = (uint32_t)(e - sg[s].base);
            uint32_t in_seg = 1;
            if (sg[s].kind == 0) {
                const size_t r = (size_t)sg[s].src + j;
                const uint32_t row = j / sg[s].degree;
                a[k] = nbr[r] + sg[s].lvl; b[k] = row + sg[s].off; in_seg = j - row * sg[s].degree + 1;
                w[k] = w32 ? fmake(w32[r]) : wF[r];
            } else { a[k] = j + sg[s].lvl; b[k] = j + sg[s].off; w[k] = minus1; }
            c2[k] = cell_count2(sg, s, b[k]) + in_seg;
        }
        reinterpret_cast<uint4 *>(idx1)[q] = make_uint4(a[0], a[1], a[2], a[3]);
        reinterpret_cast<uint4 *>(idx2)[q] = make_uint4(b[0], b[1], b[2], b[3]);
        reinterpret_cast<uint4 *>(cnt2)[q] = make_uint4(c2[0], c2[1], c2[2], c2[3]);
        for (int k = 0; k < 4; k++) weight[e0 + k] = w[k];
    }
}
// per cell c < S = 2n: where its run starts in the sorted keys, the run's length (acc1) and the closed-form count of the idx2 cell (acc2)
__global__ void __launch_bounds__(PB) k_parity_cells(const ParitySeg *__restrict__ segs, uint32_t nseg, const uint32_t *__restrict__ skeys, size_t m, size_t S,
                                                     uint32_t *__restrict__ start, F *__restrict__ acc1, F *__restrict__ acc2) {
    __shared__ ParitySeg sg[MAX_SEGS];
    for (uint32_t i = threadIdx.x; i < nseg; i += PB) sg[i] = segs[i];
    __syncthreads();
    for (size_t c = blockIdx.x * (size_t)PB + threadIdx.x; c < S; c += (size_t)gridDim.x * PB) {
        size_t b[2];
        for (int t = 0; t < 2; t++) {                                // first sorted place whose key is >= c + t
            size_t lo = 0, hi = m;
            while (lo < hi) { const size_t mid = (lo + hi) / 2; if (skeys[mid] < (uint32_t)c + t) lo = mid + 1; else hi = mid; }
            b[t] = lo;
        }
        start[c] = (uint32_t)b[0];
        acc1[c] = fmake((uint32_t)(b[1] - b[0]));
        acc2[c] = fmake(cell_count2(sg, nseg, (uint32_t)c));
    }
}
__global__ void __launch_bounds__(PB) k_parity_cnt1(const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ spos, const uint32_t *__restrict__ start, size_t m,
                                                    uint32_t *__restrict__ cnt1) {
    for (size_t j = blockIdx.x * (size_t)PB + threadIdx.x; j < m; j += (size_t)gridDim.x * PB) cnt1[spos[j]] = (uint32_t)j - start[skeys[j]] + 1;
}

// the libc generator is part of the transcript; loading this file's code object (its first launch) must not draw from it (libcgen::Guard)
using LibcRngGuard = libcgen::Guard;

int ilog2x(size_t n) { int l = 0; while (((size_t)1 << l) < n) l++; return ((size_t)1 << l) == n ? l : -1; }

// generate_access_idx (:2622-2669) over the context's uploaded levels; returns the codeword length, -1 if a level is missing
long long access_lists(hobbit_ctx *ctx, std::vector<uint32_t> &i1, std::vector<uint32_t> &i2, std::vector<F> &w, long long Offset, long long n, int dep, long long *lvl) {
    if (n <= 13) return n;                                     // distance_threshold
    auto ci = ctx->graphs.find({dep, 0}), di = ctx->graphs.find({dep, 1});
    if (ci == ctx->graphs.end() || di == ctx->graphs.end() || ci->second.L != n) return -1;
    const HostGraph &C = ci->second, &D = di->second;
    const F minus1 = fmake(P61 - 1);
    long long R = C.R;
    for (long long i = 0; i < n; i++)
        for (int d = 0; d < C.degree; d++) { i1.push_back((uint32_t)(C.nbr[i * C.degree + d] + *lvl)); i2.push_back((uint32_t)(i + Offset)); w.push_back(C.w[i * C.degree + d]); }
    for (long long i = 0; i < R; i++) { i1.push_back((uint32_t)(*lvl + i)); i2.push_back((uint32_t)(i + Offset + n)); w.push_back(minus1); }
    long long l = *lvl + R;
    const long long L = access_lists(ctx, i1, i2, w, Offset + n, R, dep + 1, &l);
    if (L < 0 || D.L != L) return -1;
    R = D.R;
    for (long long i = 0; i < L; i++)
        for (int d = 0; d < D.degree; d++) { i1.push_back((uint32_t)(D.nbr[i * D.degree + d] + *lvl)); i2.push_back((uint32_t)(i + Offset + n)); w.push_back(D.w[i * D.degree + d]); }
    for (long long i = 0; i < R; i++) { i1.push_back((uint32_t)(i + *lvl)); i2.push_back((uint32_t)(i + Offset + n + L)); w.push_back(minus1); }
    *lvl += R;
    return n + L + R;
}

}  // namespace

struct hobbit_parity_commitment : hobbit_ctx::ParityBufs {       // the five device buffers: d_u32, d_F, d_pw, d_enc, d_levels
    hobbit_ctx *ctx; long long n; size_t m, P; double list_seconds;
    // pinned host copies of what was uploaded: the uploads are queued (asynchronous from pinned memory), so their sources live as long as the object
    mem::Buf<uint32_t, mem::Pinned> h_u32; mem::Buf<F, mem::Pinned> h_F;
    int alloc_device() {
        const size_t S = 2 * (size_t)n, W = P;                 // W: encoded row length 2 * 8P / 16
        return d_u32.alloc(4 * P) || d_F.alloc(P + 2 * S) || d_pw.alloc(8 * P) || d_enc.alloc(16 * W) || d_levels.alloc(64 * W);
    }
    const uint32_t *idx1() const { return d_u32; }
    const uint32_t *idx2() const { return d_u32 + P; }
    const uint32_t *cnt1() const { return d_u32 + 2 * P; }
    const uint32_t *cnt2() const { return d_u32 + 3 * P; }
    const F *weight() const { return d_F; }
    const F *acc1() const { return d_F + P; }
    const F *acc2() const { return d_F + P + 2 * (size_t)n; }
};

extern "C" {

void hobbit_parity_commitment_free(hobbit_parity_commitment *c) {
    if (!c) return;
    hipSetDevice(c->ctx->device);
    hipStreamSynchronize(c->ctx->stream);
    if (c->whole() && !c->ctx->spare_parity.d_u32) {             // park a whole set for the next device-built commit
        c->ctx->spare_parity = std::move(static_cast<hobbit_ctx::ParityBufs &>(*c));
        c->ctx->spare_parity_P = c->P; c->ctx->spare_parity_n = c->n;
    }
    delete c;
}

int hobbit_parity_commit(hobbit_ctx *ctx, long long n, hobbit_parity_commitment **out) {
    if (!out) return ctx->fail(HOBBIT_EINVAL, "parity_commit: null output");
    *out = nullptr;
    if (n < 16 || n > (1LL << CODE_MAX_LOG) || (n & (n - 1))) return ctx->fail(HOBBIT_EINVAL, "parity_commit: n must be a power of two in [16, 2^21]");
    if (ctx->code.n != n) return ctx->fail(HOBBIT_ESTATE, "parity_commit: graphs for this n are not finalized (hobbit_graph_finalize)");
    const size_t S = 2 * (size_t)n;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> i1, i2; std::vector<F> w;
    long long lvl = 0;
    const long long len = access_lists(ctx, i1, i2, w, 0, n, 0, &lvl);
    if (len < 0 || len != ctx->code.len) return ctx->fail(HOBBIT_ESTATE, "parity_commit: the uploaded levels do not form the code of this n");
    const size_t m = i1.size();
    size_t P = 1; while (P < m) P <<= 1;
    if (m == 0 || 5 * P + 2 * S > 8 * P || 5 * P + 2 * S <= 4 * P) return ctx->fail(HOBBIT_EINVAL, "parity_commit: list length outside the public witness' 8P layout");
    LibcRngGuard guard;
    hipSetDevice(ctx->device);
    if (parity_is_long(P)) HB_TRY(need_device_bytes(ctx, parity_commit_bytes(P, S), "parity_commit"));
    Handle<hobbit_parity_commitment, hobbit_parity_commitment_free> c(new hobbit_parity_commitment());
    c->ctx = ctx; c->n = n; c->m = m; c->P = P;
    if (c->h_u32.alloc(4 * P) || c->h_F.alloc(P + 2 * S)) return ctx->fail(HOBBIT_ENOMEM, "parity_commit: pinned host allocation failed");
    memset(c->h_u32, 0, 4 * P * sizeof(uint32_t)); memset((void *)c->h_F.get(), 0, (P + 2 * S) * sizeof(F));
    {
        std::vector<uint32_t> a1(S, 0), a2(S, 0);
        for (size_t i = 0; i < m; i++) {
            if (i1[i] >= S || i2[i] >= S) { return ctx->fail(HOBBIT_EINVAL, "parity_commit: list index beyond the 2n cells"); }
            c->h_u32[i] = i1[i]; c->h_u32[P + i] = i2[i];
            c->h_u32[2 * P + i] = ++a1[i1[i]]; c->h_u32[3 * P + i] = ++a2[i2[i]];
            c->h_F[i] = w[i];
        }
        for (size_t i = 0; i < S; i++) { c->h_F[P + i] = fmake(a1[i]); c->h_F[P + S + i] = fmake(a2[i]); }
    }
    c->list_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (c->alloc_device()) return ctx->fail(HOBBIT_ENOMEM, "parity_commit: device allocation failed");
    int rc = ctx->hip(hipMemcpyAsync(c->d_u32, c->h_u32, 4 * P * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream), "parity_commit: upload");
    if (!rc) rc = ctx->hip(hipMemcpyAsync(c->d_F, c->h_F, (P + 2 * S) * sizeof(F), hipMemcpyHostToDevice, ctx->stream), "parity_commit: upload");
    if (!rc) {
        ctx->prof_begin("k_parity_witness");
        hipLaunchKernelGGL(k_parity_witness, dim3(pgrid(8 * P)), dim3(PB), 0, ctx->stream, c->idx1(), c->idx2(), c->cnt1(), c->cnt2(), c->weight(), c->acc1(), c->acc2(), m, P, m,
                           S, c->d_pw);
        ctx->prof_end("k_parity_witness");
        rc = ctx->hip(hipGetLastError(), "k_parity_witness");
    }
    if (!rc) rc = hobbit_shockwave_commit(ctx, aF(c->d_pw), 8 * P, 16, aF(c->d_enc), c->d_levels);
    if (rc) return rc;
    *out = c.release();
    return 0;
}

int hobbit_parity_dims(const hobbit_parity_commitment *c, long long *n, size_t *m, size_t *P, double *list_seconds) {
    if (!c) return HOBBIT_EINVAL;
    if (n) *n = c->n;
    if (m) *m = c->m;
    if (P) *P = c->P;
    if (list_seconds) *list_seconds = c->list_seconds;
    return 0;
}
const void *hobbit_parity_dev(const hobbit_parity_commitment *c, int which) {
    if (!c) return nullptr;
    switch (which) {
        case 0: return c->idx1(); case 1: return c->idx2(); case 2: return c->cnt1(); case 3: return c->cnt2(); case 4: return c->weight();
        case 5: return c->acc1(); case 6: return c->acc2(); case 7: return c->d_pw; case 8: return c->d_enc; case 9: return c->d_levels;
    }
    return nullptr;
}
int hobbit_parity_root(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint8_t *h_root) {
    if (!c || !h_root) return ctx->fail(HOBBIT_EINVAL, "parity_root: null argument");
    return hobbit_memcpy_d2h(ctx, h_root, c->d_levels + 32 * (2 * c->P - 2), 32);
}
int hobbit_parity_levels(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint8_t *h_levels) {
    if (!c || !h_levels) return ctx->fail(HOBBIT_EINVAL, "parity_levels: null argument");
    return hobbit_memcpy_d2h(ctx, h_levels, c->d_levels, 32 * (2 * c->P - 1));
}
int hobbit_parity_lists(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint32_t *h_idx1, uint32_t *h_idx2, uint32_t *h_cnt1, uint32_t *h_cnt2, hobbit_F *h_weight,
                        hobbit_F *h_acc1, hobbit_F *h_acc2) {
    if (!c) return ctx->fail(HOBBIT_EINVAL, "parity_lists: null commitment");
    const size_t P = c->P, S = 2 * (size_t)c->n;
    uint32_t *hu[4] = {h_idx1, h_idx2, h_cnt1, h_cnt2};
    for (int k = 0; k < 4; k++) if (hu[k]) HB_TRY(hobbit_memcpy_d2h(ctx, hu[k], c->d_u32 + k * P, P * sizeof(uint32_t)));
    if (h_weight) HB_TRY(hobbit_memcpy_d2h(ctx, h_weight, c->weight(), P * sizeof(F)));
    if (h_acc1) HB_TRY(hobbit_memcpy_d2h(ctx, h_acc1, c->acc1(), S * sizeof(F)));
    if (h_acc2) HB_TRY(hobbit_memcpy_d2h(ctx, h_acc2, c->acc2(), S * sizeof(F)));
    return 0;
}

namespace {
inline F q2_claim(CHP q) { return fadd(fadd(q[0], q[1]), fadd(q[2], q[2])); }     // q(0) + q(1) of a x^2 + b x + c
}  // namespace

int hobbit_parity_open(hobbit_ctx *ctx, const hobbit_parity_commitment *c, const hobbit_F *h_r1, const hobbit_F *h_r2, int rlen, hobbit_parity_open_out *o) {
    if (!c || !h_r1 || !h_r2 || !o || !o->sp_p || !o->sp_w) return ctx->fail(HOBBIT_EINVAL, "parity_open: null argument");
    if (c->ctx != ctx) return ctx->fail(HOBBIT_EINVAL, "parity_open: the commitment belongs to another context");
    const size_t P = c->P, m = c->m, S = 2 * (size_t)c->n;
    const int L = ilog2x(P), l = ilog2x(S);
    if (rlen != l) return ctx->fail(HOBBIT_EINVAL, "parity_open: rlen must be log2(2n)");
    if (L < 12 || L > 26 || L <= l) return ctx->fail(HOBBIT_EINVAL, "parity_open: needs 2^12 <= P <= 2^26 (n = 128 .. 2^21): the nested WHIR proofs take widths 2^9 .. 2^25");
    if (parity_is_long(P)) HB_TRY(need_device_bytes(ctx, parity_open_bytes(P), "parity_open"));      // (before the first draw)
    Scratch sc(ctx);
    F *beta1, *beta2, *betas12, *rows, *encw, *eq, *part, *pw2; uint8_t *lvw;
    const uint32_t nb = pgrid(m, 1024);
    HB_TRY(sc.get(2 * S * sizeof(F), (void **)&beta1)); beta2 = beta1 + S;
    HB_TRY(sc.get(2 * P * sizeof(F), (void **)&betas12));
    HB_TRY(sc.get(4 * P * sizeof(F), (void **)&rows));
    HB_TRY(sc.get(4 * P * sizeof(F), (void **)&encw));                              // C_w: 16 x 2 (2P / 16)
    HB_TRY(sc.get(64 * (P / 4), (void **)&lvw));                                    // its tree: 2 W - 1 hashes, W = P / 4
    HB_TRY(sc.get((P + 7 * (size_t)nb + 8) * sizeof(F), (void **)&eq)); part = eq + P;
    HB_TRY(sc.get(8 * P * sizeof(F), (void **)&pw2));
    const F one = fmake(1);
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](int k) {                                                        // every stage ends in a host-returning call: the stream is drained here
        const auto t = std::chrono::steady_clock::now();
        if (o->stage_ms) o->stage_ms[k] = std::chrono::duration<double, std::milli>(t - t_last).count();
        t_last = t;
    };

    HB_TRY(hobbit_eq_table(ctx, h_r1, l, aF(beta1)));                                // precompute_beta(r1), (r2) (:2715-2716)
    HB_TRY(hobbit_eq_table(ctx, h_r2, l, aF(beta2)));
    const F a = fmake((uint64_t)random()), b = fmake((uint64_t)random());            // (:2748-2749); shockwave_commit (:2742) draws nothing
    ctx->prof_begin("k_parity_gather");
    hipLaunchKernelGGL(k_parity_gather, dim3(pgrid(P)), dim3(PB), 0, ctx->stream, c->idx1(), c->idx2(), c->cnt1(), c->cnt2(), beta1, beta2, a, b, m, P, betas12, rows);
    ctx->prof_end("k_parity_gather");
    HB_CHECK(ctx, hipGetLastError());
    HB_TRY(hobbit_shockwave_commit(ctx, aF(betas12), 2 * P, 16, aF(encw), lvw));     // C_w (:2740-2742)
    HB_TRY(hobbit_memcpy_d2h(ctx, o->cw_root, lvw + 32 * (2 * (P / 4) - 2), 32));
    hobbit_F p21 = {21, 0}, p321 = {321, 0};
    stage(0);
    HB_TRY(hobbit_mul_tree(ctx, aF(rows), 4, P, &p21, nullptr, o->t1_cpoly, o->t1_r, o->t1_vr, o->t1_fin, o->t1_final_r, o->t1_evals, o->t1_evals + 1, o->t1_layers));   // P1 (:2767)
    std::vector<F> ind((size_t)L);                                                   // P1.individual_randomness = final_r[0 .. log2 P)
    for (int i = 0; i < L; i++) ind[(size_t)i] = cF(o->t1_final_r)[i];
    stage(1);

    HB_TRY(hobbit_eq_table(ctx, aF(ind.data()), L, aF(eq)));                         // (:2768-2780)
    ctx->prof_begin("k_parity_eval");
    hipLaunchKernelGGL(k_parity_eval, dim3(nb), dim3(PB), 0, ctx->stream, eq, c->idx1(), c->idx2(), c->cnt1(), c->cnt2(), c->weight(), betas12, m, P, part);
    hipLaunchKernelGGL(k_parity_eval_final, dim3(1), dim3(PB), 0, ctx->stream, part, nb, part + 7 * (size_t)nb);
    ctx->prof_end("k_parity_eval");
    HB_CHECK(ctx, hipGetLastError());
    F py[8];
    HB_TRY(hobbit_memcpy_d2h(ctx, py, part + 7 * (size_t)nb, 7 * sizeof(F)));
    for (int k = 0; k < 7; k++) mF(o->partial)[k] = py[k];

    ctx->prof_begin("k_parity_tree2");
    hipLaunchKernelGGL(k_parity_tree2, dim3(pgrid(S)), dim3(PB), 0, ctx->stream, beta1, beta2, c->acc1(), c->acc2(), a, b, S, rows);
    ctx->prof_end("k_parity_tree2");
    HB_CHECK(ctx, hipGetLastError());
    HB_TRY(hobbit_mul_tree(ctx, aF(rows), 4, S, &p21, nullptr, o->t2_cpoly, o->t2_r, o->t2_vr, o->t2_fin, o->t2_final_r, o->t2_evals, o->t2_evals + 1, o->t2_layers));   // (:2796)

    F y_acc1, y_acc2;                                                                // (:2800-2813)
    HB_TRY(hobbit_eval_vector(ctx, aF(c->acc1()), S, aF(ind.data()), aF(&y_acc1)));
    HB_TRY(hobbit_eval_vector(ctx, aF(c->acc2()), S, aF(ind.data()), aF(&y_acc2)));
    mF(o->acc_y)[0] = y_acc1; mF(o->acc_y)[1] = y_acc2;
    F p5 = fadd(fmul(y_acc1, fsub(one, ind[(size_t)l])), fmul(y_acc2, ind[(size_t)l]));
    for (int i = l + 1; i < L; i++) p5 = fmul(p5, fsub(one, ind[(size_t)i]));
    stage(2);

    HB_TRY(hobbit_sumcheck3(ctx, aF(c->weight()), aF(betas12), aF(betas12 + P), P, &p321, o->p2_cpoly, o->p2_r, o->p2_vr, o->p2_fin));      // P2 (:2819)
    const F r = fmake((uint64_t)random()), a_ = fmake((uint64_t)random());           // (:2822)
    mF(o->scalars)[0] = a; mF(o->scalars)[1] = b; mF(o->scalars)[2] = r; mF(o->scalars)[3] = a_;
    const F vr0 = cF(o->p2_vr)[0], vr1 = cF(o->p2_vr)[1], vr2 = cF(o->p2_vr)[2];
    F y1 = fadd(fmul(fsub(one, r), py[5]), fmul(r, py[6])), y2 = fadd(fmul(fsub(one, r), vr1), fmul(r, vr2));
    std::vector<F> ra(ind), rb((size_t)L);
    for (int i = 0; i < L; i++) rb[(size_t)i] = cF(o->p2_r)[i];
    ra.push_back(r); rb.push_back(r);
    const F al[2] = {one, a_};
    HB_TRY(hobbit_sumcheck2_eq(ctx, 2, aF(ra.data()), aF(rb.data()), aF(al), aF(betas12), 2 * P, &p321, o->p3_qpoly, o->p3_r, o->p3_vr, o->p3_fin));   // P3 (:2837)
    o->checks[0] = feq(q2_claim(cF(o->p3_qpoly)), fadd(y1, fmul(a_, y2))) ? 1 : 0;   // "Error 1"

    ctx->prof_begin("k_parity_witness");                                             // the open layout: idx2 at P (:2846-2858)
    hipLaunchKernelGGL(k_parity_witness, dim3(pgrid(8 * P)), dim3(PB), 0, ctx->stream, c->idx1(), c->idx2(), c->cnt1(), c->cnt2(), c->weight(), c->acc1(), c->acc2(), m, P, P, S,
                       pw2);
    ctx->prof_end("k_parity_witness");
    HB_CHECK(ctx, hipGetLastError());
    F pad[3];
    hobbit_generate_randomness(3, aF(pad));                                          // aggr_r_pad (:2861)
    F pv[8] = {py[0], py[1], py[2], py[3], py[4], p5, fmake(0), fmake(0)};           // pad_vector(partial_y1); evaluate_vector (:2863)
    for (int i = 0; i < 3; i++) for (int j = 0; j < (4 >> i); j++) pv[j] = fadd(fmul(fsub(one, pad[i]), pv[2 * j]), fmul(pad[i], pv[2 * j + 1]));
    y1 = pv[0]; y2 = vr0;
    ra.assign(ind.begin(), ind.end()); ra.insert(ra.end(), pad, pad + 3);
    rb.resize((size_t)L); rb.push_back(fmake(0)); rb.push_back(fmake(0)); rb.push_back(one);
    HB_TRY(hobbit_sumcheck2_eq(ctx, 2, aF(ra.data()), aF(rb.data()), aF(al), aF(pw2), 8 * P, &p321, o->p4_qpoly, o->p4_r, o->p4_vr, o->p4_fin));       // P4 (:2875)
    o->checks[1] = feq(q2_claim(cF(o->p4_qpoly)), fadd(y1, fmul(a_, y2))) ? 1 : 0;   // "Error 2"
    stage(3);

    HB_TRY(hobbit_shockwave_prove(ctx, aF(c->d_pw), aF(c->d_enc), c->d_levels, 8 * P, 16, o->p4_r, L + 3, o->sp_p));     // (:2881)
    stage(4);
    HB_TRY(hobbit_shockwave_prove(ctx, aF(betas12), aF(encw), lvw, 2 * P, 16, o->p3_r, L + 1, o->sp_w));                 // (:2883)
    stage(5);
    return 0;
}

int hobbit_prove_linear_code_batch(hobbit_ctx *ctx, const hobbit_F *d_codewords, size_t count, size_t ld, size_t len, long long n, const hobbit_F *h_r1,
                                   const hobbit_F *h_r2, hobbit_F *h_qpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    if (!d_codewords || !h_r1 || !h_r2) return ctx->fail(HOBBIT_EINVAL, "prove_linear_code_batch: null argument");
    const int lc = ilog2x(count);
    if (n < 1 || (n & (n - 1)) || lc < 1 || len > 2 * (size_t)n || ld < len) return ctx->fail(HOBBIT_EINVAL, "prove_linear_code_batch: n a power of two, count a power of two >= 2, len <= 2n, ld >= len");
    if (ctx->code.n != n) return ctx->fail(HOBBIT_ESTATE, "prove_linear_code_batch: graphs for this n are not finalized");
    const size_t S = 2 * (size_t)n; const int l = ilog2x(S);
    Scratch sc(ctx);
    F *beta, *A, *B, *beta2;
    HB_TRY(sc.get((3 * S + count) * sizeof(F), (void **)&beta)); A = beta + S; B = A + S; beta2 = B + S;
    HB_TRY(hobbit_eq_table(ctx, h_r1, l, aF(beta)));
    HB_TRY(hobbit_eq_table(ctx, h_r2, lc, aF(beta2)));
    HB_TRY(hobbit_parity_matrix(ctx, aF(beta), S, n, aF(A)));
    LibcRngGuard guard;                                                              // this file's first launch may be this one
    ctx->prof_begin("k_parity_batch_rows");
    hipLaunchKernelGGL(k_parity_batch_rows, dim3(pgrid(S)), dim3(PB), 0, ctx->stream, reinterpret_cast<const F *>(d_codewords), count, ld, len, beta2, S, B);
    ctx->prof_end("k_parity_batch_rows");
    HB_CHECK(ctx, hipGetLastError());
    return hobbit_sumcheck2(ctx, aF(A), aF(B), S, h_r1 + (l - 1), h_qpoly, h_r, h_vr, h_final);
}

// ---- include/hobbit_parity_lists.h ----------------------------------------------------------------------------------------------------------------
int hobbit_parity_shape(hobbit_ctx *ctx, long long n, size_t *m_out, size_t *P_out) {
    if (n < 16 || n > (1LL << CODE_MAX_LOG) || (n & (n - 1))) return ctx->fail(HOBBIT_EINVAL, "parity_commit: n must be a power of two in [16, 2^21]");
    if (ctx->code.n != n) return ctx->fail(HOBBIT_ESTATE, "parity_commit: graphs for this n are not finalized (hobbit_graph_finalize)");
    std::vector<ParitySeg> segs; size_t m = 0;
    HB_TRY(parity_segments(ctx, segs, &m));
    const size_t S = 2 * (size_t)n;
    size_t P = 1; while (P < m) P <<= 1;
    if (m == 0 || segs.size() > MAX_SEGS || 5 * P + 2 * S > 8 * P) return ctx->fail(HOBBIT_EINVAL, "parity_commit: list length outside the public witness' 8P layout");
    if (m_out) *m_out = m;
    if (P_out) *P_out = P;
    return 0;
}

int hobbit_parity_commit_device(hobbit_ctx *ctx, long long n, hobbit_parity_commitment **out) {
    if (!out) return ctx->fail(HOBBIT_EINVAL, "parity_commit: null output");
    *out = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    size_t m = 0, P = 0;
    HB_TRY(hobbit_parity_shape(ctx, n, &m, &P));
    LibcRngGuard guard;
    hipSetDevice(ctx->device);
    HB_TRY(ensure_fwd(ctx));
    const DeviceCode &code = ctx->code;
    const size_t S = 2 * (size_t)n;
    const uint32_t nseg = (uint32_t)code.fwd_segs.size();
    Scratch sc(ctx);
    uint32_t *skeys, *spos, *start; void *tmp = nullptr; size_t tmp_bytes = 0;
    Handle<hobbit_parity_commitment, hobbit_parity_commitment_free> c(new hobbit_parity_commitment());
    c->ctx = ctx; c->n = n; c->m = m; c->P = P;
    hobbit_ctx::ParityBufs &own = *c;
    if (ctx->spare_parity.d_u32 && ctx->spare_parity_P == P && ctx->spare_parity_n == n) {          // the buffers of a retired commitment of this shape
        own = std::move(ctx->spare_parity);
    } else {
        if (ctx->spare_parity.d_u32) { hipStreamSynchronize(ctx->stream); ctx->spare_parity = {}; }   // another shape: release it before allocating
        if (parity_is_long(P)) HB_TRY(need_device_bytes(ctx, parity_commit_bytes(P, S), "parity_commit"));
        if (c->alloc_device()) return ctx->fail(HOBBIT_ENOMEM, "parity_commit: device allocation failed");
    }
    uint32_t *idx1 = c->d_u32, *idx2 = idx1 + P, *cnt1 = idx2 + P, *cnt2 = cnt1 + P;
    int rc = sc.get((2 * m + S) * sizeof(uint32_t), (void **)&skeys);
    if (rc) return rc;
    spos = skeys + m; start = spos + m;
    const rocprim::counting_iterator<uint32_t> places(0);
    const unsigned key_bits = (unsigned)ilog2x(S);                  // every idx1 is below 2n (ensure_fwd)
    rc = ctx->hip(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const uint32_t *)idx1, skeys, places, spos, m, 0u, key_bits, ctx->stream), "parity_commit: sort scratch");
    if (!rc) rc = sc.get(tmp_bytes, &tmp);
    if (rc) return rc;
    rc = ctx->hip(hipMemsetAsync(cnt1 + m, 0, (P - m) * sizeof(uint32_t), ctx->stream), "parity_commit: cnt1 padding");
    if (rc) return rc;
    ctx->prof_begin("k_parity_fill");
    hipLaunchKernelGGL(k_parity_fill, dim3(pgrid(P / 4)), dim3(PB), 0, ctx->stream, code.d_fwd_segs, nseg, code.d_fwd_nbr, code.d_fwd_w32, code.d_fwd_w, m, P, idx1, idx2, cnt2,
                       c->d_F);
    ctx->prof_end("k_parity_fill");
    rc = ctx->hip(hipGetLastError(), "k_parity_fill");
    if (rc) return rc;
    ctx->prof_begin("k_parity_sort");
    rc = ctx->hip(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint32_t *)idx1, skeys, places, spos, m, 0u, key_bits, ctx->stream), "parity_commit: sort");
    ctx->prof_end("k_parity_sort");
    if (rc) return rc;
    ctx->prof_begin("k_parity_cnt1");
    hipLaunchKernelGGL(k_parity_cells, dim3(pgrid(S)), dim3(PB), 0, ctx->stream, code.d_fwd_segs, nseg, skeys, m, S, start, c->d_F + P, c->d_F + P + S);
    hipLaunchKernelGGL(k_parity_cnt1, dim3(pgrid(m)), dim3(PB), 0, ctx->stream, skeys, spos, start, m, cnt1);
    ctx->prof_end("k_parity_cnt1");
    rc = ctx->hip(hipGetLastError(), "k_parity_cnt1");
    if (rc) return rc;
    c->list_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ctx->prof_begin("k_parity_witness");
    hipLaunchKernelGGL(k_parity_witness, dim3(pgrid(8 * P)), dim3(PB), 0, ctx->stream, c->idx1(), c->idx2(), c->cnt1(), c->cnt2(), c->weight(), c->acc1(), c->acc2(), m, P, m, S,
                       c->d_pw);
    ctx->prof_end("k_parity_witness");
    rc = ctx->hip(hipGetLastError(), "k_parity_witness");
    if (!rc) rc = hobbit_shockwave_commit(ctx, aF(c->d_pw), 8 * P, 16, aF(c->d_enc), c->d_levels);
    if (rc) return rc;
    *out = c.release();
    return 0;
}

}  // extern "C"
