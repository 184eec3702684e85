/* hobbit_orion.h -- fifth header of libhobbit_hip.so: the Orion comparison baseline, test_PC option 2
 * (src/Our_PC.cpp:28-65 _compute_tensorcode_linear_code, 173-195 commit_standard_orion, 523-602 open_orion_standard;
 * src/PC_utils.cpp:150-166 recursive_prover_orion).  The uncalled GKR variant (_recursive_prover_orion, src/Our_PC.cpp:309-353) is not built.
 *
 * N = 2^n coefficients, n even, B = 2^(n/2).  The commitment is an expander x expander tensor code: the B x B message (row i =
 * poly[i B .. (i + 1) B)) becomes a 2B x 2B row-major matrix T -- every message row encoded to width 2B (codeword, then zeros), then every column
 * (its first B entries) encoded in place -- and one MT_commit_Blake over the flattened 4N elements (N leaves of four consecutive F, then the
 * tree).  The opening draws Q = min(B, 4096) pairs (I[q], J[q]), gathers the Q queried columns of T (the reference re-encodes their message
 * halves; the field is exact and the encode deterministic, so that is column I[q] of T bit for bit), commits them (C = shockwave_commit(arr, 32)),
 * proves them codewords in a batch against the committed parity matrix, opens C at the batch proof's point and opens the Q^2 grid of leaves.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_ORION_H
#define HOBBIT_ORION_H
#include "hobbit_hip.h"
#include "hobbit_parity.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hobbit_orion hobbit_orion;

#define HOBBIT_ORION_MAX_QUERIES 4096        /* src/Our_PC.cpp:548-552 */

/* ---- the three device pieces the baseline adds, callable on their own ------------------------------------------------------------------ */
/* hobbit_encode_interleaved in place on a 2n x ld matrix (element (i, c) of message / codeword i at d_mat[c * ld + i]), for the messages
 * i < width only: width any positive integer <= ld, neither a power of two.  For those i entries c < n are read, n <= c < len written with the
 * codeword and len <= c < 2n with zeros; entries i >= width of every row are neither read nor written.  2 n roundup(width, 64) < 2^31; graphs
 * for n finalized (else HOBBIT_ESTATE).  Bit-identical to hobbit_encode_interleaved and hobbit_encode_batch. */
int hobbit_encode_interleaved_ld(hobbit_ctx *ctx, hobbit_F *d_mat, long long n, size_t width, size_t ld);
/* the same with the grid order chosen by the caller (measurement surface): strip = 0 walks all `width` messages of a few outputs together, as
 * hobbit_encode_interleaved does; strip = a multiple of 64 walks every output of a step over `strip` messages before the next strip.  The
 * result does not depend on it. */
int hobbit_encode_interleaved_ld_order(hobbit_ctx *ctx, hobbit_F *d_mat, long long n, size_t width, size_t ld, uint32_t strip);
/* d_arr[q * nrows + c] = d_T[c * ld + h_I[q]] for q < nq, c < nrows: nq columns of a row-major matrix, each laid out as a row.  h_I[q] < ld
 * (else HOBBIT_EINVAL before any launch); duplicates are allowed.  The transposition goes through an LDS tile: the writes are coalesced. */
int hobbit_orion_gather(hobbit_ctx *ctx, const hobbit_F *d_T, size_t nrows, size_t ld, const uint32_t *h_I, size_t nq, hobbit_F *d_arr);
/* open_tree_blake(MT, {I[i], J[j]}, cols) for every pair, i outer: the sibling path of leaf (h_J[j] / 4) * cols + h_I[i] of the flat levels over
 * n leaves (n a power of two) into d_paths[(i * nq + j) * log2 n * 32 ...], a DEVICE buffer of nq^2 log2(n) 32 B.  The positions are computed
 * on the device; every one is checked on the host against n from max I and max J before the launch (HOBBIT_EINVAL). */
int hobbit_orion_grid_paths(hobbit_ctx *ctx, const uint8_t *d_levels, size_t n, size_t cols, const uint32_t *h_I, const uint32_t *h_J, size_t nq, uint8_t *d_paths);

/* ---- the baseline ------------------------------------------------------------------------------------------------------------------------- */
/* Shapes served: N = 2^n, n even, 14 <= n <= 28 (below: B < 128, the parity opening's smallest code; above: not in PC_tests.sh; odd n: the
 * reference encodes rows of length B with graphs drawn for 2B).  Anything else is HOBBIT_EINVAL.  B = 2^(n/2), Q = min(B, 4096).  Host only;
 * B and Q may be NULL. */
int hobbit_orion_shape(size_t N, size_t *B, size_t *Q);

/* commit_standard_orion on d_poly (N F, device): rows by hobbit_encode_batch, columns by hobbit_encode_interleaved_ld over the first `len`
 * columns (the others are zero before and after the pass; this call writes their zeros), leaves and tree by hobbit_mt_commit_blake.  Every
 * entry of the 2B x 2B tensor is written.  Graphs for n = B finalized (else HOBBIT_ESTATE; the reference draws them inside the commitment,
 * expander_init_store(B), after the polynomial).  A refused shape is HOBBIT_EINVAL before any allocation or launch.  Asynchronous on the
 * context's stream, as hobbit_commit_standard; draws nothing from libc. */
int hobbit_orion_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, hobbit_orion **out);
void hobbit_orion_free(hobbit_orion *c);
int hobbit_orion_dims(const hobbit_orion *c, size_t *N, size_t *B, size_t *Q, long long *len);                  /* len: codeword length */
const hobbit_F *hobbit_orion_tensor_dev(const hobbit_orion *c);                  /* device, 2B x 2B row-major */
const uint8_t *hobbit_orion_levels_dev(const hobbit_orion *c);                   /* device, flat levels: N leaves ... root, (2N - 1) x 32 B */
int hobbit_orion_root(hobbit_ctx *ctx, const hobbit_orion *c, uint8_t *h_root);

/* open_orion_standard, prover side, returned synchronised.  h_x (xlen F): the point; the reference computes precompute_beta of its first
 * n/2 coordinates and reads nothing of it, so no value of the opening depends on x (xlen >= n/2 is still required).
 * libc draws stay on the host, in the reference's order: r_v[0] = generate_randomness(1) (drawn, its powers feed nothing); Q pairs
 * I[q] = rand() % 2B, J[q] = rand() % 2B, interleaved; both before anything is queued; then generate_randomness(log2 2B) and
 * generate_randomness(log2 Q) of prove_linear_code_batch; the draws hobbit_parity_open documents; those of shockwave_prove(C, .).
 * Stages (stage_ms, host wall time, every stage ends synchronised):
 *   0  arr = the Q queried columns back to back (Q x 2B), C = shockwave_commit(arr, 32);
 *   1  commit_parity_matrix(B) (hobbit_parity_commit_device);
 *   2  P1 = prove_linear_code_batch(codewords, B);
 *   3  open_parity_matrix(P1.randomness[0], r1, B);
 *   4  shockwave_prove(C, P1.randomness[0] | r2);
 *   5  the Q^2 paths, pair (i, j) at index i Q + j: open_tree_blake(MT, {I[i], J[j]}, 2B).
 * The commitment of another context, graphs finalized for another n (HOBBIT_ESTATE) or a NULL argument are refused before any draw,
 * allocation or launch.  parity and sp_c (with the buffers hobbit_parity_open / hobbit_shockwave_prove ask for, N = 2 B Q, k = 32) are
 * required, the others may be NULL.  All are host buffers but d_paths:
 *   I, J (Q each), c_root, cp_root (32 B: roots of C and C_p; C_w's is parity->cw_root),
 *   p1_* : P1 as hobbit_sumcheck2 lays it out (log2 2B rounds), p1_r1 / p1_r2 its drawn challenge vectors (log2 2B and log2 Q F),
 *   d_paths : DEVICE buffer of Q^2 x log2 N x 32 B, or NULL: the paths are not produced (at 2^28 they are 2^24 paths, 15 GB); a caller reads
 *             any range back with hobbit_memcpy_d2h,
 *   stage_ms : 6 doubles. */
typedef struct {
    uint32_t *I, *J; uint8_t *c_root, *cp_root;
    hobbit_F *p1_qpoly, *p1_r, *p1_vr, *p1_fin, *p1_r1, *p1_r2;
    hobbit_parity_open_out *parity;
    hobbit_shockwave_out *sp_c;
    uint8_t *d_paths;
    double *stage_ms;
} hobbit_orion_open_out;
int hobbit_orion_open(hobbit_ctx *ctx, const hobbit_orion *c, const hobbit_F *h_x, int xlen, hobbit_orion_open_out *out);

/* The proof size in KB as the reference accumulates it from 0 (:570-571, :588-595), from a finished opening: P1, the parity opening,
 * shockwave_prove(C), the constant 2^20 F of :571, and per pair 2 F plus verify_claim_opt_blake at position (J[j] / 2) B + I[i] / 2 (as
 * written: not the position that was opened).  `visited` is an uninitialised new bool[] in the reference; it is taken as all false here.
 * Accounting, not proving: host only, outside the opening's stage times (at 2^28 it walks 2^24 positions of a 2^29-entry table).  Needs I, J
 * and the query outputs (I, wqidx, wqn, iters) of sp_c, parity->sp_p, parity->sp_w and the trees' layer counts (else HOBBIT_EINVAL). */
int hobbit_orion_proof_size(const hobbit_orion *c, const hobbit_orion_open_out *out, size_t parity_P, double *ps);

#ifdef __cplusplus
}
#endif
#endif
