// hobbit_orion.hip -- the C ABI of include/hobbit_orion.h: the Orion baseline, test_PC option 2 (src/Our_PC.cpp:28-65, 173-195, 523-602;
// src/PC_utils.cpp:150-166).  Two kernels of its own -- the gather of the queried columns and the grid of opening paths; the strided
// rows-innermost encode sits beside k_enc_ilv in hobbit_kernels.hip, whose arithmetic it shares -- and otherwise a sequence of the library's
// entry points in the reference's order, so that the libc draws each of them takes fall where the reference's do.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>
#include "hobbit_kernels.hpp"
#include "hobbit_libcgen.hpp"
#include "../../include/hobbit_orion.h"
#include "../../include/hobbit_parity_lists.h"
#include "hobbit_ps.hpp"

using namespace hobbit;
using namespace hobbit_ps;

static inline const hobbit_F *aF(const F *p) { return reinterpret_cast<const hobbit_F *>(p); }
static inline hobbit_F *aF(F *p) { return reinterpret_cast<hobbit_F *>(p); }

namespace {

// the libc generator is part of the transcript; loading this file's code object (its first launch) must not draw from it (libcgen::Guard)
using LibcRngGuard = libcgen::Guard;

// arr[q][c] = T[c][I[q]]: a workgroup moves a tile of GT columns c x GT queries q.  It reads with q fastest -- the 16-byte entries of one row
// of T at the queried positions, a gather by nature: the positions are random -- and writes with c fastest, 512 contiguous bytes per half
// wave, the transposition going through LDS (rows padded by one F against bank conflicts).
constexpr uint32_t GT = 32;
__global__ void __launch_bounds__(256)
k_orion_gather(const F *__restrict__ T, size_t nrows, size_t ld, const uint32_t *__restrict__ I, size_t nq, F *__restrict__ arr) {
    __shared__ uint4 tile[GT][GT + 1];                          // [q][c]
    const size_t c0 = (size_t)blockIdx.x * GT, q0 = (size_t)blockIdx.y * GT;
    const uint32_t lo = threadIdx.x % GT, hi = threadIdx.x / GT;
    const size_t q = q0 + lo;
    const size_t col = q < nq ? I[q] : 0;
    for (uint32_t cc = hi; cc < GT; cc += 256 / GT)
        if (q < nq && c0 + cc < nrows) tile[lo][cc] = *reinterpret_cast<const uint4 *>(T + (c0 + cc) * ld + col);
    __syncthreads();
    for (uint32_t qq = hi; qq < GT; qq += 256 / GT)
        if (q0 + qq < nq && c0 + lo < nrows) *reinterpret_cast<uint4 *>(arr + (q0 + qq) * nrows + c0 + lo) = tile[qq][lo];
}

// paths[(i nq + j)][l] = levels[off_l + ((J[j] / 4) cols + I[i] >> l) ^ 1], off_l = 2n - (2n >> l) (n a power of two): one thread per
// (pair, level), levels fastest, so a path's `depth` digests are written by neighbouring lanes  (src/merkle_tree.cpp:308-324)
__global__ void __launch_bounds__(256)
k_orion_grid_paths(const uint8_t *__restrict__ levels, size_t n, size_t cols, const uint32_t *__restrict__ I, const uint32_t *__restrict__ J, size_t nq,
                   uint32_t depth, uint8_t *__restrict__ paths) {
    const size_t total = nq * nq * depth;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t pair = g / depth; const uint32_t l = (uint32_t)(g - pair * depth);
        const size_t i = pair / nq, j = pair - i * nq;
        const size_t pos = (size_t)(J[j] / 4) * cols + I[i];
        const size_t off = 2 * n - ((2 * n) >> l);
        const uint4 *s = reinterpret_cast<const uint4 *>(levels + 32 * (off + ((pos >> l) ^ 1)));
        uint4 *d = reinterpret_cast<uint4 *>(paths + 32 * g);
        d[0] = s[0]; d[1] = s[1];
    }
}

int launch_orion_gather(hobbit_ctx *ctx, const F *T, size_t nrows, size_t ld, const uint32_t *d_I, size_t nq, F *arr) {
    if (!nrows || !nq) return 0;
    LibcRngGuard guard;
    HB_LAUNCH(ctx, "k_orion_gather", k_orion_gather, dim3((unsigned)((nrows + GT - 1) / GT), (unsigned)((nq + GT - 1) / GT)), dim3(256), 0, T, nrows, ld, d_I, nq, arr);
    return 0;
}
int launch_orion_grid_paths(hobbit_ctx *ctx, const uint8_t *levels, size_t n, size_t cols, const uint32_t *d_I, const uint32_t *d_J, size_t nq, int depth,
                            uint8_t *d_paths) {
    const size_t total = nq * nq * (size_t)depth;
    if (!total) return 0;
    LibcRngGuard guard;
    const size_t blocks = std::min((total + 255) / 256, (size_t)1 << 22);
    HB_LAUNCH(ctx, "k_orion_grid_paths", k_orion_grid_paths, dim3((unsigned)blocks), dim3(256), 0, levels, n, cols, d_I, d_J, nq, (uint32_t)depth, d_paths);
    return 0;
}

// every position (J[j] / 4) cols + I[i] lies below n, and every I below cols
bool grid_in_range(const uint32_t *I, const uint32_t *J, size_t nq, size_t cols, size_t n) {
    if (!nq) return true;
    const size_t mi = *std::max_element(I, I + nq), mj = *std::max_element(J, J + nq);
    return mi < cols && (mj / 4) * cols + mi < n;
}

}  // namespace

struct hobbit_orion {
    hobbit_ctx *ctx; size_t N, B, Q; long long len;
    Scratch mem; F *d_T = nullptr; uint8_t *d_levels = nullptr;      // `mem` owns: 2B x 2B row-major | flat levels over the N leaves, (2N - 1) x 32 B
};

extern "C" {

int hobbit_encode_interleaved_ld_order(hobbit_ctx *ctx, hobbit_F *d_mat, long long n, size_t width, size_t ld, uint32_t strip) {
    if (n <= 0 || !d_mat || width == 0 || width > ld || (size_t)2 * n * ((width + 63) / 64 * 64) >= ((size_t)1 << 31) || strip % 64)
        return ctx->fail(HOBBIT_EINVAL, "encode_interleaved_ld: 0 < width <= ld, 2 n roundup(width, 64) < 2^31, strip a multiple of 64");
    if (ctx->code.n != n) return ctx->fail(HOBBIT_ESTATE, "encode_interleaved_ld: graphs for this n are not finalized (hobbit_graph_finalize)");
    HB_TRY(ensure_ilv(ctx));
    return launch_encode_ilv_ld(ctx, reinterpret_cast<F *>(d_mat), (uint32_t)width, ld, strip);
}
// The order the library runs with: strip-major over 64 columns.  Measured against the plain order on the 2B x 2B buffer of the commitment, in
// one process, alternating (Orion; profiles/orion.json): 0.78 / 3.28 / 14.5 ms against 1.14 / 5.26 / 23.7 ms at 2^24 / 2^26 /
// 2^28, every run within 1 % of its median; 128 and 256 columns are 3 % and 11 % slower than 64.
static constexpr uint32_t ORION_ENC_STRIP = 64;
int hobbit_encode_interleaved_ld(hobbit_ctx *ctx, hobbit_F *d_mat, long long n, size_t width, size_t ld) {
    return hobbit_encode_interleaved_ld_order(ctx, d_mat, n, width, ld, ORION_ENC_STRIP);
}

int hobbit_orion_gather(hobbit_ctx *ctx, const hobbit_F *d_T, size_t nrows, size_t ld, const uint32_t *h_I, size_t nq, hobbit_F *d_arr) {
    if (!d_T || !d_arr || (nq && !h_I)) return ctx->fail(HOBBIT_EINVAL, "orion_gather: null argument");
    for (size_t q = 0; q < nq; q++) if (h_I[q] >= ld) return ctx->fail(HOBBIT_EINVAL, "orion_gather: column index out of range");
    if (!nq || !nrows) return 0;
    Scratch sc(ctx); uint32_t *d_I;
    HB_TRY(sc.get(nq * 4, (void **)&d_I));
    HB_TRY(hobbit_memcpy_h2d(ctx, d_I, h_I, nq * 4));
    HB_TRY(launch_orion_gather(ctx, reinterpret_cast<const F *>(d_T), nrows, ld, d_I, nq, reinterpret_cast<F *>(d_arr)));
    return ctx->sync();                                                                 // the index buffer is released on return
}

int hobbit_orion_grid_paths(hobbit_ctx *ctx, const uint8_t *d_levels, size_t n, size_t cols, const uint32_t *h_I, const uint32_t *h_J, size_t nq, uint8_t *d_paths) {
    if (!d_levels || !d_paths || (nq && (!h_I || !h_J))) return ctx->fail(HOBBIT_EINVAL, "orion_grid_paths: null argument");
    const int depth = ilog2x(n);
    if (depth < 0) return ctx->fail(HOBBIT_EINVAL, "orion_grid_paths: n must be a power of two");
    if (!grid_in_range(h_I, h_J, nq, cols, n)) return ctx->fail(HOBBIT_EINVAL, "orion_grid_paths: position out of range");   // src/merkle_tree.cpp:310-313
    if (!nq || !depth) return 0;
    Scratch sc(ctx); uint32_t *d_IJ;
    HB_TRY(sc.get(2 * nq * 4, (void **)&d_IJ));
    HB_TRY(hobbit_memcpy_h2d(ctx, d_IJ, h_I, nq * 4));
    HB_TRY(hobbit_memcpy_h2d(ctx, d_IJ + nq, h_J, nq * 4));
    HB_TRY(launch_orion_grid_paths(ctx, d_levels, n, cols, d_IJ, d_IJ + nq, nq, depth, d_paths));
    return ctx->sync();
}

int hobbit_orion_shape(size_t N, size_t *B, size_t *Q) {
    const int n = ilog2x(N);
    if (N == 0 || n < 14 || n > 28 || (n & 1)) return HOBBIT_EINVAL;
    const size_t b = (size_t)1 << (n / 2);
    if (B) *B = b;
    if (Q) *Q = std::min(b, (size_t)HOBBIT_ORION_MAX_QUERIES);
    return 0;
}

void hobbit_orion_free(hobbit_orion *c) { delete c; }

int hobbit_orion_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, hobbit_orion **out) {
    if (!out) return ctx->fail(HOBBIT_EINVAL, "orion_commit: null output");
    *out = nullptr;
    size_t B, Q;
    if (hobbit_orion_shape(N, &B, &Q)) return ctx->fail(HOBBIT_EINVAL, "orion_commit: N = 2^n, n even, 14 <= n <= 28");
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "orion_commit: null polynomial");
    if (ctx->code.n != (long long)B) return ctx->fail(HOBBIT_ESTATE, "orion_commit: graphs for n = sqrt(N) are not finalized (expander_init_store(sqrt(N)))");
    const size_t S = 2 * B; const size_t len = (size_t)ctx->code.len;
    Handle<hobbit_orion, hobbit_orion_free> c(new hobbit_orion{ctx, N, B, Q, ctx->code.len, Scratch(ctx)});
    int r = c->mem.get(S * S * sizeof(F), (void **)&c->d_T);
    if (!r) r = c->mem.get((2 * N - 1) * 32, (void **)&c->d_levels);
    // rows: message row i to row i of T, all 2B entries written (codeword, then zeros)
    if (!r) r = hobbit_encode_batch(ctx, d_poly, aF(c->d_T), (long long)B, B, B, S);
    // columns: the first B entries of every column encoded in place.  Columns from len on are zero in every message row, so their codewords
    // are zero: they are written here and left out of the pass
    if (!r) r = launch_zero_rect(ctx, c->d_T, S, B, B, len, S - len);
    if (!r) r = hobbit_encode_interleaved_ld(ctx, aF(c->d_T), (long long)B, len, S);
    if (!r) r = hobbit_mt_commit_blake(ctx, aF(c->d_T), 4 * N, c->d_levels);
    if (r) return r;
    *out = c.release();
    return 0;
}

int hobbit_orion_dims(const hobbit_orion *c, size_t *N, size_t *B, size_t *Q, long long *len) {
    if (!c) return HOBBIT_EINVAL;
    if (N) *N = c->N;
    if (B) *B = c->B;
    if (Q) *Q = c->Q;
    if (len) *len = c->len;
    return 0;
}
const hobbit_F *hobbit_orion_tensor_dev(const hobbit_orion *c) { return c ? aF(c->d_T) : nullptr; }
const uint8_t *hobbit_orion_levels_dev(const hobbit_orion *c) { return c ? c->d_levels : nullptr; }
int hobbit_orion_root(hobbit_ctx *ctx, const hobbit_orion *c, uint8_t *h_root) {
    if (!c || !h_root) return ctx->fail(HOBBIT_EINVAL, "orion_root: null argument");
    return hobbit_memcpy_d2h(ctx, h_root, c->d_levels + 32 * (2 * c->N - 2), 32);
}

int hobbit_orion_open(hobbit_ctx *ctx, const hobbit_orion *c, const hobbit_F *h_x, int xlen, hobbit_orion_open_out *o) {
    if (!c || !h_x || !o || !o->parity || !o->sp_c) return ctx->fail(HOBBIT_EINVAL, "orion_open: null argument (parity and sp_c are required)");
    if (c->ctx != ctx) return ctx->fail(HOBBIT_EINVAL, "orion_open: the commitment belongs to another context");
    if (!o->parity->sp_p || !o->parity->sp_w) return ctx->fail(HOBBIT_EINVAL, "orion_open: parity needs sp_p and sp_w");
    const size_t B = c->B, Q = c->Q, S = 2 * B, N = c->N;
    const int l = ilog2x(S), lq = ilog2x(Q), ln = ilog2x(N);
    if (xlen < ln / 2) return ctx->fail(HOBBIT_EINVAL, "orion_open: the point has fewer than log2(N) / 2 coordinates");
    if (ctx->code.n != (long long)B) return ctx->fail(HOBBIT_ESTATE, "orion_open: graphs for n = sqrt(N) are not finalized (expander_init_store(sqrt(N)))");

    // ---- the draws that come before any device work (:540, :547-558; precompute_beta(x1) feeds nothing) -----------------------------------------
    hobbit_F rv0; hobbit_generate_randomness(1, &rv0); (void)rv0;                       // r_v[0]: its powers feed nothing
    std::vector<uint32_t> IJ(2 * Q);                                                    // I | J
    for (size_t q = 0; q < Q; q++) { IJ[q] = (uint32_t)(rand() % (long)S); IJ[Q + q] = (uint32_t)(rand() % (long)S); }
    if (o->I) std::copy(IJ.begin(), IJ.begin() + Q, o->I);
    if (o->J) std::copy(IJ.begin() + Q, IJ.end(), o->J);

    Scratch sc(ctx);
    const size_t NC = Q * S, W_c = 2 * (NC / 32);                                       // C: 32 rows of Q S / 32, encoded to Q S / 16
    F *arr, *enc; uint8_t *lvc; uint32_t *d_IJ;
    HB_TRY(sc.get(2 * Q * 4, (void **)&d_IJ));
    HB_TRY(sc.get(NC * sizeof(F), (void **)&arr));
    HB_TRY(sc.get(2 * NC * sizeof(F), (void **)&enc));
    HB_TRY(sc.get(64 * W_c, (void **)&lvc));
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](int k) -> int {
        HB_TRY(ctx->sync());
        const auto t = std::chrono::steady_clock::now();
        if (o->stage_ms) o->stage_ms[k] = std::chrono::duration<double, std::milli>(t - t_last).count();
        t_last = t;
        return 0;
    };

    // ---- 0: the queried columns (:560-568: their re-encode is column I[q] of the tensor), C (src/PC_utils.cpp:153-157) -------------------------
    HB_TRY(hobbit_memcpy_h2d(ctx, d_IJ, IJ.data(), 2 * Q * 4));
    HB_TRY(launch_orion_gather(ctx, c->d_T, S, S, d_IJ, Q, arr));
    HB_TRY(hobbit_shockwave_commit(ctx, aF(arr), NC, 32, aF(enc), lvc));
    if (o->c_root) HB_TRY(hobbit_memcpy_d2h(ctx, o->c_root, lvc + 32 * (2 * W_c - 2), 32));
    HB_TRY(stage(0));

    // ---- 1: commit_parity_matrix(B) (:160) ------------------------------------------------------------------------------------------------------
    ParityHandle pc;
    { hobbit_parity_commitment *p = nullptr; HB_TRY(hobbit_parity_commit_device(ctx, (long long)B, &p)); pc.reset(p); }
    if (o->cp_root) HB_TRY(hobbit_parity_root(ctx, pc.get(), o->cp_root));
    HB_TRY(stage(1));

    // ---- 2: P1 = prove_linear_code_batch (:161; src/sumcheck.cpp:3201-3221: r1, then r2) ----------------------------------------------------------
    std::vector<F> r1((size_t)l), r2((size_t)lq), q((size_t)3 * l), r((size_t)l + lq); F vr[2], fin;
    hobbit_generate_randomness((size_t)l, aF(r1.data()));
    hobbit_generate_randomness((size_t)lq, aF(r2.data()));
    HB_TRY(hobbit_prove_linear_code_batch(ctx, aF(arr), Q, S, S, (long long)B, aF(r1.data()), aF(r2.data()), aF(q.data()), aF(r.data()), aF(vr), aF(&fin)));
    {
        MHP pq(reinterpret_cast<HF *>(o->p1_qpoly)), pr(reinterpret_cast<HF *>(o->p1_r)), pv(reinterpret_cast<HF *>(o->p1_vr)), pf(reinterpret_cast<HF *>(o->p1_fin)),
            p1(reinterpret_cast<HF *>(o->p1_r1)), p2(reinterpret_cast<HF *>(o->p1_r2));
        if (pq) for (size_t i = 0; i < q.size(); i++) pq[i] = q[i];
        if (pr) for (int i = 0; i < l; i++) pr[(size_t)i] = r[(size_t)i];
        if (pv) { pv[0] = vr[0]; pv[1] = vr[1]; }
        if (pf) pf[0] = fin;
        if (p1) for (int i = 0; i < l; i++) p1[(size_t)i] = r1[(size_t)i];
        if (p2) for (int i = 0; i < lq; i++) p2[(size_t)i] = r2[(size_t)i];
    }
    HB_TRY(stage(2));

    // ---- 3: open_parity_matrix(P1.randomness[0], P1.randomness[1], B) (:163) ----------------------------------------------------------------------
    HB_TRY(hobbit_parity_open(ctx, pc.get(), aF(r.data()), aF(r1.data()), l, o->parity));
    HB_TRY(stage(3));

    // ---- 4: shockwave_prove(C, P1.randomness[0] | r2) (:164-165) -----------------------------------------------------------------------------------
    for (int i = 0; i < lq; i++) r[(size_t)l + i] = r2[(size_t)i];
    HB_TRY(hobbit_shockwave_prove(ctx, aF(arr), aF(enc), lvc, NC, 32, aF(r.data()), l + lq, o->sp_c));
    HB_TRY(stage(4));

    // ---- 5: open_tree_blake(MT, {I[i], J[j]}, 2B) for every pair, i outer (:574-580) ----------------------------------------------------------------
    if (o->d_paths) {
        if (!grid_in_range(IJ.data(), IJ.data() + Q, Q, S, N)) return ctx->fail(HOBBIT_EINVAL, "orion_open: position out of range");
        HB_TRY(launch_orion_grid_paths(ctx, c->d_levels, N, S, d_IJ, d_IJ + Q, Q, ln, o->d_paths));
    }
    HB_TRY(stage(5));
    return 0;
}

int hobbit_orion_proof_size(const hobbit_orion *c, const hobbit_orion_open_out *o, size_t P, double *out) {
    if (!c || !o || !out || !o->I || !o->J || !o->parity || P == 0 || ilog2x(P) < 0) return HOBBIT_EINVAL;
    if (!(sp_has_queries(o->sp_c) && sp_has_queries(o->parity->sp_p) && sp_has_queries(o->parity->sp_w) && o->parity->t1_layers && o->parity->t2_layers))
        return HOBBIT_EINVAL;
    const size_t B = c->B, Q = c->Q, S = 2 * B, N = c->N;
    const int l = ilog2x(S), L = ilog2x(P), ln = ilog2x(N);
    double ps = 0.0;
    sumcheck2_ps(l, ps);                                                                // prove_linear_code_batch
    for (int k = 0; k < *o->parity->t1_layers; k++) sumcheck3_ps(2 + k, ps);            // open_parity_matrix: both trees, P2, P3, P4, C_p, C_w
    for (int k = 0; k < *o->parity->t2_layers; k++) sumcheck3_ps(2 + k, ps);
    sumcheck3_ps(L, ps); sumcheck2_ps(L + 1, ps); sumcheck2_ps(L + 3, ps);
    shockwave_ps(o->parity->sp_p, 8 * P, 16, ps); shockwave_ps(o->parity->sp_w, 2 * P, 16, ps);
    shockwave_ps(o->sp_c, Q * S, 32, ps);
    ps += (double)(((size_t)1 << 20) * sizeof(hobbit_F)) / 1024.0;                      // (:571)
    // (:588-595) per pair 2 F and verify_claim_opt_blake at (J[j] / 2) B + I[i] / 2, `visited` all false at the start
    std::vector<bool> visited(2 * N + 2, false);
    for (size_t i = 0; i < Q; i++)
        for (size_t j = 0; j < Q; j++) {
            ps += 2 * FKB;
            size_t pe = N + (size_t)(o->J[j] / 2) * B + o->I[i] / 2;
            for (int k = 0; k < ln; k++) {
                if (visited[pe ^ 1]) break;
                visited[pe ^ 1] = true; pe /= 2; visited[pe] = true;
                ps += 32.0 / 1024.0;
            }
        }
    *out = ps;
    return 0;
}

}  // extern "C"
