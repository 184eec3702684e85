// hobbit_brakingbase.hip -- the C ABI of include/hobbit_brakingbase.h: the Braking base baseline, test_PC option 5 (src/Our_PC.cpp:114-144,
// 238-256, 355-429; src/PC_utils.cpp:389-394).  No kernel of its own: the commitment is hobbit_brakedown_commit's body at the shape
// (trs, K), and the opening is a sequence of the library's entry points in the reference's order, so that the libc draws each of them takes
// fall where the reference's do.
#include <chrono>
#include <cstdlib>
#include <vector>
#include "hobbit_kernels.hpp"
#include "../../include/hobbit_brakingbase.h"
#include "../../include/hobbit_parity_lists.h"
#include "../../include/hobbit_longcodes.h"
#include "hobbit_ps.hpp"

using namespace hobbit;
using namespace hobbit_ps;

static inline const hobbit_F *aF(const F *p) { return reinterpret_cast<const hobbit_F *>(p); }
static inline hobbit_F *aF(F *p) { return reinterpret_cast<hobbit_F *>(p); }

namespace {

constexpr size_t QUERIES = HOBBIT_BRAKINGBASE_QUERIES;
constexpr int CAP_LOG = 20;                                     // hobbit_brakingbase.h: trs <= 2^20; hobbit_longcodes.h: trs <= 2^CODE_MAX_LOG

// the shape rule of both headers: N, K powers of two, 4 <= K <= 512, 128 <= N / K <= 2^cap_log
bool shape_k_ok(size_t N, size_t K) { return ilog2x(N) >= 0 && ilog2x(K) >= 0 && K >= 4 && K <= 512 && N >= K; }
int shape_capped(size_t N, size_t K, int cap_log, size_t *trs) {
    if (!shape_k_ok(N, K)) return HOBBIT_EINVAL;
    const size_t t = N / K;
    if (t < 128 || t > ((size_t)1 << cap_log)) return HOBBIT_EINVAL;
    if (trs) *trs = t;
    return 0;
}

}  // namespace

struct hobbit_brakingbase {
    hobbit_ctx *ctx; size_t N, K, trs;
    Handle<hobbit_brakedown, hobbit_brakedown_free> bd;     // the matrix (2 trs x K, rows-innermost) and the levels over its 2 trs column digests
};

extern "C" {

int hobbit_brakingbase_shape(size_t N, size_t K, size_t *trs) { return shape_capped(N, K, CAP_LOG, trs); }
int hobbit_brakingbase_shape_any(size_t N, size_t K, size_t *trs) { return shape_capped(N, K, CODE_MAX_LOG, trs); }

void hobbit_brakingbase_free(hobbit_brakingbase *c) { delete c; }

}  // extern "C"

// the body of both commits; cap_log and the two refusal messages are the export's own
static int commit_capped(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, size_t K, int left_left_quirk, hobbit_brakingbase **out, int cap_log, const char *too_long,
                         const char *bad_shape) {
    if (!out) return ctx->fail(HOBBIT_EINVAL, "brakingbase_commit: null output");
    *out = nullptr;
    size_t trs;
    if (shape_capped(N, K, cap_log, &trs)) {
        if (shape_k_ok(N, K) && N / K > ((size_t)1 << cap_log)) return ctx->fail(HOBBIT_EINVAL, too_long);
        return ctx->fail(HOBBIT_EINVAL, bad_shape);
    }
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "brakingbase_commit: null polynomial");
    if (ctx->code.n != (long long)trs) return ctx->fail(HOBBIT_ESTATE, "brakingbase_commit: graphs for n = N / K are not finalized (expander_init_store(N / K))");
    // the matrix (2 trs x K) and its levels; past 2^20 the device is asked first (the machines are shared)
    if (trs > ((size_t)1 << CAP_LOG)) HB_TRY(need_device_bytes(ctx, 2 * trs * K * sizeof(F) + 4 * trs * 32, "brakingbase_commit_any"));
    hobbit_brakedown *bd = nullptr;
    HB_TRY(brakedown_commit_shape(ctx, reinterpret_cast<const F *>(d_poly), trs, (uint32_t)K, left_left_quirk, &bd));
    *out = new hobbit_brakingbase{ctx, N, K, trs, Handle<hobbit_brakedown, hobbit_brakedown_free>(bd)};
    return 0;
}

extern "C" {

int hobbit_brakingbase_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, size_t K, int left_left_quirk, hobbit_brakingbase **out) {
    return commit_capped(ctx, d_poly, N, K, left_left_quirk, out, CAP_LOG,
                         "brakingbase_commit: N / K above 2^20: the code proof and the parity opening stop at codes of length 2^20",
                         "brakingbase_commit: N, K powers of two, 4 <= K <= 512, 128 <= N / K <= 2^20");
}
int hobbit_brakingbase_commit_any(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, size_t K, int left_left_quirk, hobbit_brakingbase **out) {
    return commit_capped(ctx, d_poly, N, K, left_left_quirk, out, CODE_MAX_LOG,
                         "brakingbase_commit_any: N / K above 2^21: at 2^22 the parity matrix' encoded rows hold 2^31 elements, a size this library has not been verified at",
                         "brakingbase_commit_any: N, K powers of two, 4 <= K <= 512, 128 <= N / K <= 2^21");
}

int hobbit_brakingbase_dims(const hobbit_brakingbase *c, size_t *N, size_t *K, size_t *trs, long long *len) {
    if (!c) return HOBBIT_EINVAL;
    if (N) *N = c->N;
    if (K) *K = c->K;
    if (trs) *trs = c->trs;
    return hobbit_brakedown_dims(c->bd.get(), nullptr, nullptr, len);
}
const hobbit_F *hobbit_brakingbase_matrix_dev(const hobbit_brakingbase *c) { return c ? hobbit_brakedown_matrix_dev(c->bd.get()) : nullptr; }
const uint8_t *hobbit_brakingbase_levels_dev(const hobbit_brakingbase *c) { return c ? hobbit_brakedown_levels_dev(c->bd.get()) : nullptr; }
int hobbit_brakingbase_levels(hobbit_ctx *ctx, const hobbit_brakingbase *c, uint8_t *h_levels) {
    if (!c || !h_levels) return ctx->fail(HOBBIT_EINVAL, "brakingbase_levels: null argument");
    return hobbit_brakedown_levels(ctx, c->bd.get(), h_levels);
}
int hobbit_brakingbase_root(hobbit_ctx *ctx, const hobbit_brakingbase *c, uint8_t *h_root) {
    if (!c || !h_root) return ctx->fail(HOBBIT_EINVAL, "brakingbase_root: null argument");
    return hobbit_brakedown_root(ctx, c->bd.get(), h_root);
}
int hobbit_brakingbase_tensor(hobbit_ctx *ctx, const hobbit_brakingbase *c, size_t col_lo, size_t ncols, hobbit_F *h_out) {
    if (!c || (ncols && !h_out)) return ctx->fail(HOBBIT_EINVAL, "brakingbase_tensor: null argument");
    return hobbit_brakedown_tensor(ctx, c->bd.get(), col_lo, ncols, h_out);
}

}  // extern "C"

// the body of both openings: cap_log is the export's own limit on the commitment it takes
static int open_capped(hobbit_ctx *ctx, const hobbit_brakingbase *c, const hobbit_F *h_x, hobbit_brakingbase_open_out *o, int cap_log) {
    if (!c || !h_x || !o || !o->parity || !o->sp_c) return ctx->fail(HOBBIT_EINVAL, "brakingbase_open: null argument (parity and sp_c are required)");
    if (c->trs > ((size_t)1 << cap_log)) return ctx->fail(HOBBIT_EINVAL, "brakingbase_open: a commitment of hobbit_brakingbase_commit_any with N / K above 2^20 is opened by hobbit_brakingbase_open_any");
    if (c->ctx != ctx) return ctx->fail(HOBBIT_EINVAL, "brakingbase_open: the commitment belongs to another context");
    if (!o->parity->sp_p || !o->parity->sp_w) return ctx->fail(HOBBIT_EINVAL, "brakingbase_open: parity needs sp_p and sp_w");
    if (o->ps && !(sp_has_queries(o->sp_c) && sp_has_queries(o->parity->sp_p) && sp_has_queries(o->parity->sp_w) && o->parity->t1_layers && o->parity->t2_layers))
        return ctx->fail(HOBBIT_EINVAL, "brakingbase_open: ps needs the query outputs (I, wqidx, wqn, iters) of sp_c, parity->sp_p, parity->sp_w and the trees' layer counts");
    const size_t trs = c->trs, K = c->K, S = 2 * trs;
    const int lk = ilog2x(K), l = ilog2x(S);
    if (ctx->code.n != (long long)trs) return ctx->fail(HOBBIT_ESTATE, "brakingbase_open: graphs for n = N / K are not finalized (expander_init_store(N / K))");
    const F *mat = reinterpret_cast<const F *>(hobbit_brakedown_matrix_dev(c->bd.get()));
    const uint8_t *levels = hobbit_brakedown_levels_dev(c->bd.get());
    if (trs > ((size_t)1 << CAP_LOG)) {
        // the parity matrix committed and opened inside this call: asked of the device before the first draw
        size_t P = 0;
        HB_TRY(hobbit_parity_shape(ctx, (long long)trs, nullptr, &P));
        if (parity_is_long(P)) HB_TRY(need_device_bytes(ctx, parity_commit_bytes(P, S) + parity_open_bytes(P), "brakingbase_open_any"));
    }

    // ---- the draws that come before any device work (:374, :382-385; _aggregate_brakingbase and shockwave_commit draw nothing) -----------------
    hobbit_F rv0; hobbit_generate_randomness(1, &rv0); (void)rv0;                       // r_v[0]: its powers feed nothing
    std::vector<uint32_t> I(QUERIES);
    for (size_t q = 0; q < QUERIES; q++) I[q] = (uint32_t)(rand() % (long)S);
    if (o->I) for (size_t q = 0; q < QUERIES; q++) o->I[q] = I[q];

    Scratch sc(ctx);
    const size_t w_c = S / 32, W_c = 2 * w_c;                                            // C_c: 32 rows of trs / 16, encoded to trs / 8
    F *beta, *aggr, *cw, *enc, *rep; uint8_t *lvc, *pth; uint32_t *d_I; uint64_t *d_pos;
    HB_TRY(sc.get((K + 2 * trs) * sizeof(F), (void **)&beta)); aggr = beta + K;         // (aggr | the unused second sum of k_bd_aggr)
    HB_TRY(sc.get(S * sizeof(F), (void **)&cw));
    HB_TRY(sc.get(2 * S * sizeof(F), (void **)&enc));
    HB_TRY(sc.get(64 * W_c, (void **)&lvc));
    HB_TRY(sc.get(QUERIES * K * sizeof(F), (void **)&rep));
    HB_TRY(sc.get(QUERIES * (size_t)l * 32, (void **)&pth));
    HB_TRY(sc.get(QUERIES * 4, (void **)&d_I));
    HB_TRY(sc.get(QUERIES * 8, (void **)&d_pos));
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](int k) -> int {
        HB_TRY(ctx->sync());
        const auto t = std::chrono::steady_clock::now();
        if (o->stage_ms) o->stage_ms[k] = std::chrono::duration<double, std::milli>(t - t_last).count();
        t_last = t;
        return 0;
    };

    // ---- 0: beta, the aggregate over the message columns, its codeword, C_c (:372, :238-256) ---------------------------------------------------
    HB_TRY(hobbit_eq_table(ctx, h_x, lk, aF(beta)));
    HB_TRY(launch_brakedown_aggr(ctx, mat, (uint32_t)K, trs, beta, beta, aggr, aggr + trs));
    HB_TRY(ensure_ilv(ctx));
    HB_TRY(launch_copy(ctx, cw, aggr, trs * sizeof(F)));
    HB_TRY(launch_encode_ilv(ctx, cw, cw, 1));                                          // encode_monolithic: one row of the rows-innermost encode
    HB_TRY(hobbit_shockwave_commit(ctx, aF(cw), S, 32, aF(enc), lvc));
    if (o->aggr) HB_TRY(hobbit_memcpy_d2h(ctx, o->aggr, aggr, trs * sizeof(F)));
    if (o->cc_root) HB_TRY(hobbit_memcpy_d2h(ctx, o->cc_root, lvc + 32 * (2 * W_c - 2), 32));
    HB_TRY(stage(0));

    // ---- 1: replies and paths (:386-399) --------------------------------------------------------------------------------------------------------
    if (o->reply) {
        HB_TRY(hobbit_memcpy_h2d(ctx, d_I, I.data(), QUERIES * 4));
        HB_TRY(launch_brakedown_reply(ctx, mat, (uint32_t)K, d_I, QUERIES, rep));
        HB_TRY(hobbit_memcpy_d2h(ctx, o->reply, rep, QUERIES * K * sizeof(F)));
    }
    if (o->paths) {
        // open_tree_blake(MT, {0, I[q]}, 0) takes leaf (I[q] / 4) * 0 + 0: every path is leaf 0's
        std::vector<uint64_t> pos(QUERIES);
        for (size_t q = 0; q < QUERIES; q++) pos[q] = (I[q] / 4) * 0 + 0;
        HB_TRY(hobbit_memcpy_h2d(ctx, d_pos, pos.data(), QUERIES * 8));
        HB_TRY(launch_merkle_paths(ctx, levels, S, d_pos, QUERIES, l, pth));
        HB_TRY(hobbit_memcpy_d2h(ctx, o->paths, pth, QUERIES * (size_t)l * 32));
    }
    HB_TRY(stage(1));

    // ---- recursive_prover_brakingbase (src/PC_utils.cpp:389-394) ----------------------------------------------------------------------------------
    ParityHandle pc;
    { hobbit_parity_commitment *p = nullptr; HB_TRY(hobbit_parity_commit_device(ctx, (long long)trs, &p)); pc.reset(p); }
    if (o->cp_root) HB_TRY(hobbit_parity_root(ctx, pc.get(), o->cp_root));
    HB_TRY(stage(2));

    std::vector<F> r1((size_t)l), q((size_t)3 * l), r((size_t)l); F vr[2], fin;
    hobbit_generate_randomness((size_t)l, aF(r1.data()));                               // prove_linear_code's own draw (src/sumcheck.cpp:3225)
    HB_TRY(hobbit_prove_linear_code(ctx, aF(cw), S, (long long)trs, aF(r1.data()), aF(q.data()), aF(r.data()), aF(vr), aF(&fin)));
    {
        MHP pq(reinterpret_cast<HF *>(o->p1_qpoly)), pr(reinterpret_cast<HF *>(o->p1_r)), pv(reinterpret_cast<HF *>(o->p1_vr)), pf(reinterpret_cast<HF *>(o->p1_fin)),
            p1(reinterpret_cast<HF *>(o->p1_r1));
        if (pq) for (size_t i = 0; i < q.size(); i++) pq[i] = q[i];
        if (pr) for (int i = 0; i < l; i++) pr[(size_t)i] = r[(size_t)i];
        if (pv) { pv[0] = vr[0]; pv[1] = vr[1]; }
        if (pf) pf[0] = fin;
        if (p1) for (int i = 0; i < l; i++) p1[(size_t)i] = r1[(size_t)i];
    }
    HB_TRY(stage(3));

    HB_TRY(hobbit_parity_open(ctx, pc.get(), aF(r.data()), aF(r1.data()), l, o->parity));
    HB_TRY(stage(4));
    HB_TRY(hobbit_shockwave_prove(ctx, aF(cw), aF(enc), lvc, S, 32, aF(r.data()), l, o->sp_c));
    HB_TRY(stage(5));

    if (o->ps) {
        size_t P = 0; hobbit_parity_dims(pc.get(), nullptr, nullptr, &P, nullptr);
        const int L = ilog2x(P);
        double ps = 0.0;
        ps += (double)(K * QUERIES * sizeof(hobbit_F)) / 1024.0;                        // (:393)
        ps += l * 3 * FKB + 2 * FKB;                                                    // prove_linear_code
        for (int k = 0; k < *o->parity->t1_layers; k++) sumcheck3_ps(2 + k, ps);        // open_parity_matrix: both trees, P2, P3, P4, C_p, C_w
        for (int k = 0; k < *o->parity->t2_layers; k++) sumcheck3_ps(2 + k, ps);
        sumcheck3_ps(L, ps); sumcheck2_ps(L + 1, ps); sumcheck2_ps(L + 3, ps);
        shockwave_ps(o->parity->sp_p, 8 * P, 16, ps); shockwave_ps(o->parity->sp_w, 2 * P, 16, ps);
        shockwave_ps(o->sp_c, S, 32, ps);
        path_ps(S, l, I.data(), QUERIES, ps);                                           // verify_claim_opt_blake(.., I[i], ..) (:422-424)
        *o->ps = ps;
    }
    return 0;
}

extern "C" {

int hobbit_brakingbase_open(hobbit_ctx *ctx, const hobbit_brakingbase *c, const hobbit_F *h_x, hobbit_brakingbase_open_out *o) {
    return open_capped(ctx, c, h_x, o, CAP_LOG);
}
int hobbit_brakingbase_open_any(hobbit_ctx *ctx, const hobbit_brakingbase *c, const hobbit_F *h_x, hobbit_brakingbase_open_out *o) {
    return open_capped(ctx, c, h_x, o, CODE_MAX_LOG);
}

}  // extern "C"
