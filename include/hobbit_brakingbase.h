/* hobbit_brakingbase.h -- fourth header of libhobbit_hip.so: the Braking base comparison baseline, test_PC option 5
 * (src/Our_PC.cpp:114-144 commit_brakingbase, 238-256 _aggregate_brakingbase, 355-429 open_brakingbase, 827-842 the driver;
 * src/PC_utils.cpp:389-394 recursive_prover_brakingbase).
 *
 * The commitment is Brakedown's (hobbit_brakedown_commit) at another shape: K rows of trs = N / K elements, each encoded with the code of
 * n = trs, the 2 trs columns hashed and the tree built over them.  The opening is succinct where Brakedown's is not: the beta-aggregate of the
 * rows is encoded, committed (C_c = shockwave_commit(codeword, 32)), proved a codeword (prove_linear_code), the parity matrix it was checked
 * against is committed and opened (hobbit_parity.h), and C_c is opened at the code proof's point.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_BRAKINGBASE_H
#define HOBBIT_BRAKINGBASE_H
#include "hobbit_hip.h"
#include "hobbit_parity.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hobbit_brakingbase hobbit_brakingbase;

#define HOBBIT_BRAKINGBASE_QUERIES 2935      /* src/Our_PC.cpp:360 */

/* Shapes served: N and K powers of two, 4 <= K <= 512 (MT_commit_Blake of a column needs one 64-byte leaf; the general column digest keeps
 * a stack for at most 512 rows), trs = N / K with 128 <= trs <= 2^20 (below: the parity opening's smallest n; above: these three calls keep
 * the cap they were built with -- `28 5 128` of PC_tests.sh needs a code of 2^21 and is served by the long forms of hobbit_longcodes.h,
 * `28 5 64` needs 2^22 and is refused there too).  Anything else is HOBBIT_EINVAL.  Host only; trs may be NULL. */
int hobbit_brakingbase_shape(size_t N, size_t K, size_t *trs);

/* commit_brakingbase: d_poly (N F, device) cut into K rows of trs, row i transposed into entry i of columns 0 .. trs - 1 of a 2 trs x K
 * rows-innermost matrix, every row encoded (graphs for n = trs finalized, else HOBBIT_ESTATE), every column committed with MT_commit_Blake,
 * create_tree_blake over the 2 trs digests.  left_left_quirk as hobbit_brakedown_commit.  A refused shape is HOBBIT_EINVAL before any
 * allocation or launch.  Asynchronous on the context's stream; draws nothing from libc. */
int hobbit_brakingbase_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, size_t K, int left_left_quirk, hobbit_brakingbase **out);
void hobbit_brakingbase_free(hobbit_brakingbase *c);
int hobbit_brakingbase_dims(const hobbit_brakingbase *c, size_t *N, size_t *K, size_t *trs, long long *len);    /* len: codeword length */
const hobbit_F *hobbit_brakingbase_matrix_dev(const hobbit_brakingbase *c);      /* device, 2 trs x K, element (i, c) at c * K + i */
const uint8_t *hobbit_brakingbase_levels_dev(const hobbit_brakingbase *c);       /* device, flat levels: 2 trs digests ... root */
int hobbit_brakingbase_levels(hobbit_ctx *ctx, const hobbit_brakingbase *c, uint8_t *h_levels);                 /* (4 trs - 1) x 32 B */
int hobbit_brakingbase_root(hobbit_ctx *ctx, const hobbit_brakingbase *c, uint8_t *h_root);
/* the reference's tensor[0][i][c] for every row i and c in [col_lo, col_lo + ncols): h_out[i * ncols + (c - col_lo)] (test surface) */
int hobbit_brakingbase_tensor(hobbit_ctx *ctx, const hobbit_brakingbase *c, size_t col_lo, size_t ncols, hobbit_F *h_out);

/* open_brakingbase, prover side, returned synchronised.  h_x: log2 K F (the first coordinates of the point; the reference reads no others).
 * libc draws stay on the host, in the reference's order: r_v[0] = generate_randomness(1) (drawn, never used); 2935 x rand() % (2 trs); both
 * before anything is queued; then generate_randomness(log2 2 trs) of prove_linear_code; the draws hobbit_parity_open documents; those of
 * shockwave_prove(C_c, .) (240 x rand() % (trs / 8), then _whir_prove's when trs / 16 > 256).
 * Stages (stage_ms, host wall time, every stage ends synchronised):
 *   0  beta = precompute_beta(x), aggr[j] = sum_i beta[i] poly[i trs + j] (from the matrix' message columns), codeword =
 *      encode_monolithic(aggr), C_c = shockwave_commit(codeword, 32);
 *   1  reply[q][i] = T[i][I[q]] and open_tree_blake(MT, {0, I[q]}, 0): as in Brakedown, every path is leaf 0's;
 *   2  commit_parity_matrix(trs) (inside the opening, as in the reference), the access lists built on the device
 *      (hobbit_parity_commit_device, hobbit_parity_lists.h);
 *   3  P1 = prove_linear_code(codeword, trs);
 *   4  open_parity_matrix(P1.randomness[0], P1.randomness[1], trs);
 *   5  shockwave_prove(C_c, P1.randomness[0]).
 * What the reference runs after that (:403-427) is proof-size accounting and discarded sums (its inner loop reads past beta and reply[i]);
 * only the accounting is restated.
 * The commitment of another context, graphs finalized for another n (HOBBIT_ESTATE) or a NULL argument are refused before any draw,
 * allocation or launch.  All pointers are host buffers; parity and sp_c (with the buffers hobbit_parity_open / hobbit_shockwave_prove ask
 * for, N = 2 trs, k = 32) are required, the others may be NULL:
 *   I (2935), reply (2935 x K F), paths (2935 x log2(2 trs) x 32 B), aggr (trs F), cc_root, cp_root (32 B: roots of C_c and C_p),
 *   p1_* : P1 as hobbit_sumcheck2 lays it out (log2 2 trs rounds), p1_r1 its drawn challenge vector (log2 2 trs F),
 *   ps   : the proof size in KB as the reference accumulates it from 0: the replies, P1, the parity opening, shockwave_prove(C_c),
 *          verify_claim_opt_blake fed with I[q] (needs the query outputs I / wqidx / wqn / iters of sp_c, parity->sp_p, parity->sp_w),
 *   checks : parity->checks. */
typedef struct {
    uint32_t *I; hobbit_F *reply; uint8_t *paths; hobbit_F *aggr; uint8_t *cc_root, *cp_root;
    hobbit_F *p1_qpoly, *p1_r, *p1_vr, *p1_fin, *p1_r1;
    hobbit_parity_open_out *parity;
    hobbit_shockwave_out *sp_c;
    double *ps;
    double *stage_ms;
} hobbit_brakingbase_open_out;
int hobbit_brakingbase_open(hobbit_ctx *ctx, const hobbit_brakingbase *c, const hobbit_F *h_x, hobbit_brakingbase_open_out *out);

#ifdef __cplusplus
}
#endif
#endif
