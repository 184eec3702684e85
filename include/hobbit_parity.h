/* hobbit_parity.h -- second header of libhobbit_hip.so: the succinct half of the code proof.
 *
 * prove_linear_code leaves the verifier with a claim on the code's parity-check matrix at a random point.  For the long codes (n = 8192,
 * 16384, Brakedown's 2^20) the verifier cannot evaluate that itself; the reference answers with a Spark-style opening of the matrix,
 * committed as three lists (row index, column index, weight):
 *   commit_parity_matrix (src/sumcheck.cpp:2671-2706), open_parity_matrix (:2708-2885), prove_linear_code_batch (:3201-3221).
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_PARITY_H
#define HOBBIT_PARITY_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hobbit_parity_commitment hobbit_parity_commitment;

/* commit_parity_matrix(n) for the graphs finalized for code length n (hobbit_graph_finalize(ctx, n, .), else HOBBIT_ESTATE).
 * n a power of two, 16 <= n <= 2^21 (else HOBBIT_EINVAL; at 2^21 P = 2^26, the object holds about 30 GiB, and the device is asked for the
 * memory first: HOBBIT_ENOMEM before any allocation when it is not free).  The lists of generate_access_idx (:2622-2669) are public data of the graphs: they
 * are built once per object on the host, from the levels the context holds, and uploaded.  The object owns
 *   idx1, idx2, cnt1, cnt2 : P x u32 (m entries, then zeros): A index, beta index, and the two occurrence counters (1-based: how often the
 *                            index has appeared up to and including this entry);
 *   weight                 : P F (m entries, then zeros);      acc1, acc2 : 2n F each, the final access counts of the 2n cells;
 *   C_p = shockwave_commit(public_witness, 16): the 16 x 8P/16 matrix, its encoded rows (16 x P) and the column tree (2P - 1 hashes),
 * with m the number of list entries and P the next power of two >= m.  public_witness is 8P F in the COMMIT layout (:2692-2704):
 *   idx1 at 0, idx2 at m (not P), cnt1 at 2P, cnt2 at 3P, weight at 4P, acc1 at 5P, acc2 at 5P + 2n, zeros elsewhere.
 * Asynchronous: nothing is returned through host pointers but the handle; the work is queued on the context's stream.  Draws nothing from libc. */
int hobbit_parity_commit(hobbit_ctx *ctx, long long n, hobbit_parity_commitment **out);
void hobbit_parity_commitment_free(hobbit_parity_commitment *c);
/* n, m, P; host seconds spent building the lists (any pointer may be NULL) */
int hobbit_parity_dims(const hobbit_parity_commitment *c, long long *n, size_t *m, size_t *P, double *list_seconds);
/* device pointers (use on the context's stream, or after hobbit_sync).  which: 0 idx1, 1 idx2, 2 cnt1, 3 cnt2 (u32 x P), 4 weight (F x P),
 * 5 acc1, 6 acc2 (F x 2n), 7 the matrix (F x 8P), 8 the encoded rows (F x 16P), 9 the tree levels (32 B x (2P - 1)); anything else NULL */
const void *hobbit_parity_dev(const hobbit_parity_commitment *c, int which);
int hobbit_parity_root(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint8_t *h_root);
int hobbit_parity_levels(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint8_t *h_levels);        /* (2P - 1) x 32 B, leaves first */
/* device-to-host read of the lists (test surface; any pointer may be NULL): P x u32 each, P F, 2n F each */
int hobbit_parity_lists(hobbit_ctx *ctx, const hobbit_parity_commitment *c, uint32_t *h_idx1, uint32_t *h_idx2, uint32_t *h_cnt1, uint32_t *h_cnt2,
                        hobbit_F *h_weight, hobbit_F *h_acc1, hobbit_F *h_acc2);

/* open_parity_matrix(r1, r2, n), prover side.  h_r1, h_r2: rlen = log2(2n) F each.  Everything that depends on a challenge runs on the device.
 * libc draws stay on the host, in the reference's order: a, b = F(random()); generate_randomness(2) of the first multiplication tree; that of
 * the second; r, _a = F(random()); generate_randomness(3); the draws of shockwave_prove(C_p, .); those of shockwave_prove(C_w, .).
 * The reference reads access_idx1[i] / access_idx2[i] for m <= i < P past the vectors' size (:2756-2763); this library defines those
 * entries as 0 (the reference under a zero-filling allocator).
 * The nested WHIR proofs take widths 2^9 .. 2^25 (hobbit_shockwave_prove: the table-free form above 2^24): 2^12 <= P <= 2^26, i.e.
 * n = 128 .. 2^21.  A commitment outside that range, a wrong rlen or a NULL argument is HOBBIT_EINVAL before any draw, allocation or launch.
 * At P = 2^26 the opening takes about 60 GiB of scratch and workspaces; the device is asked first (HOBBIT_ENOMEM before any draw).
 * All output pointers are host buffers (L = log2 P, l = log2 2n):
 *   t1_* / t2_*   : the two multiplication trees (4 x P and 4 x 2n) as hobbit_mul_tree lays them out; *_evals = {out_eval, final_eval};
 *   p2_*          : _generate_3product_sumcheck_proof(weight, betas1, betas2) as hobbit_sumcheck3 (L rounds);
 *   p3_* / p4_*   : the two 2-product sumchecks as hobbit_sumcheck2 (L + 1 and L + 3 rounds).  P4 runs over the OPEN layout of the public
 *                   witness (:2846-2858): as the commit layout but with idx2 at P;
 *   cw_root       : root of C_w = shockwave_commit(betas1 | betas2, 16);
 *   scalars       : a, b, r, _a;   partial : the seven inner products with eq(P1.individual_randomness) over i < m, in the order idx1, idx2,
 *                   cnt1, cnt2, weight, betas1, betas2;   acc_y : accesses1_y, accesses2_y;
 *   checks[2]     : the reference's "Error 1" / "Error 2" comparisons, 1 = holds;
 *   sp_p / sp_w   : shockwave_prove(C_p, P4.randomness) and shockwave_prove(C_w, P3.randomness), buffers as hobbit_shockwave_prove
 *                   (N = 8P and 2P, k = 16). */
typedef struct {
    hobbit_F *t1_cpoly, *t1_r, *t1_vr, *t1_fin, *t1_final_r, *t1_evals; int *t1_layers;
    hobbit_F *t2_cpoly, *t2_r, *t2_vr, *t2_fin, *t2_final_r, *t2_evals; int *t2_layers;
    hobbit_F *p2_cpoly, *p2_r, *p2_vr, *p2_fin;
    hobbit_F *p3_qpoly, *p3_r, *p3_vr, *p3_fin;
    hobbit_F *p4_qpoly, *p4_r, *p4_vr, *p4_fin;
    uint8_t *cw_root; hobbit_F *scalars, *partial, *acc_y; int *checks;
    hobbit_shockwave_out *sp_p, *sp_w;
    double *stage_ms;    /* NULL, or 6 host wall times in ms (every stage ends synchronised): eq tables + gather + C_w; first tree; evaluation
                            kernel + second tree + the two access-count evaluations; P2, P3, witness, P4; shockwave_prove(C_p); shockwave_prove(C_w) */
} hobbit_parity_open_out;
int hobbit_parity_open(hobbit_ctx *ctx, const hobbit_parity_commitment *c, const hobbit_F *h_r1, const hobbit_F *h_r2, int rlen, hobbit_parity_open_out *out);

/* prove_linear_code_batch (:3201-3221) with the challenges supplied by the caller, as in hobbit_prove_linear_code: h_r1 (log2 2n F), h_r2
 * (log2 count F).  d_codewords: `count` codewords of `len` F each (len <= 2n; the reference's B is zero past a codeword's end), codeword i at
 * d_codewords + i * ld.  count a power of two >= 2; graphs for n finalized.  B = sum_i eq(r2)[i] codeword_i, A = hobbit_parity_matrix, then
 * the 2-product sumcheck seeded with r1's last entry.  Outputs as hobbit_sumcheck2 (log2 2n rounds). */
int hobbit_prove_linear_code_batch(hobbit_ctx *ctx, const hobbit_F *d_codewords, size_t count, size_t ld, size_t len, long long n, const hobbit_F *h_r1,
                                   const hobbit_F *h_r2, hobbit_F *h_qpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final);

#ifdef __cplusplus
}
#endif
#endif
