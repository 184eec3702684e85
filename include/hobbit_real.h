/* hobbit_real.h -- a header of libhobbit_hip.so beside hobbit_whir.h and hobbit_longcodes.h: Our_PC for polynomials whose coefficients lie in
 * the BASE field F_p, p = 2^61 - 1 (every polynomial of the reference: generate_randomness returns img = 0, so do the witness streams).
 *
 * A real polynomial is `const uint64_t *`: N canonical values < p, 8 bytes each -- half the bytes of the (x, 0) form.  Two exact identities of
 * conj(a + bi) = a - bi (the Frobenius map) remove half of the commit's work ("Base-field polynomials"):
 *   rows     the 4096-point transform of a real row satisfies X[4096 - k] = conj(X[k]); columns 0 .. 2048 come from ONE 2048-point transform of
 *            the row read as 1024 F elements (x[2j] + i x[2j+1]) and an unpacking pass;
 *   columns  the drawn expander graphs have base-field weights, so column 4096 - c of a chunk's tensor is the entry-wise conjugate of column c.
 * hobbit_commit_standard_real therefore transforms, encodes and stores columns 0 .. 2048 only: a HALF commitment.  It is an
 * ordinary hobbit_commitment for every accessor of hobbit_hip.h -- root, levels, paths, tensor_row, gather answer as the full one does, bit for
 * bit -- and for hobbit_open_standard_real.  Everything here is bit-identical to the calls of hobbit_hip.h on the polynomial widened to (x, 0).
 *
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_REAL_H
#define HOBBIT_REAL_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* d_out[j] = (d_reals[j], 0), j < n: the F form of a real vector, for the calls that take one.  Asynchronous. */
int hobbit_widen_real(hobbit_ctx *ctx, const uint64_t *d_reals, hobbit_F *d_out, size_t n);

/* The row code of a real row alone: `rows` rows of 2048 reals (zero-padded to 4096 points) -> rows x 2049 F, row-major: X[0 .. 2048] of
 * hobbit_fft_batch(logn = 12) on the widened, padded row.  X[4096 - k] = conj(X[k]) gives the rest.  Asynchronous. */
int hobbit_fft_real_rows(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, hobbit_F *d_out);

/* hobbit_commit_standard of a real polynomial (16-byte aligned), same arguments, as a half commitment.  RS x expander only, and only where the
 * row code has 4096 points, 2 (N / K) / trs == 4096: every shape commit_standard is called with in the reference.  HOBBIT_EINVAL, with a
 * message that says why, before any allocation or launch: linear_time = 0 (RS x RS), another row length, or finalized graphs
 * (hobbit_graph_finalize for n = trs) with a weight whose img != 0 -- the column identity needs base-field weights.  HOBBIT_ESTATE as
 * hobbit_commit_standard where the graphs for trs > 13 are not finalized.  Asynchronous, like hobbit_commit_standard. */
int hobbit_commit_standard_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out);
/* The same from (pageable) host memory: h_poly is streamed into d_poly (N * 8 bytes, the caller's) group by group under the commit's kernels,
 * as hobbit_commit_standard_host streams 16 bytes per coefficient. */
int hobbit_commit_standard_real_host(hobbit_ctx *ctx, const uint64_t *h_poly, uint64_t *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out);

/* 1 for a commitment made by hobbit_commit_standard_real, 0 otherwise.  On a half commitment hobbit_commitment_tensor_dev materialises the full
 * linear tensor once, into an allocation of its own that the commitment owns (NULL with HOBBIT_ENOMEM recorded where the memory is not there),
 * and returns that pointer on every later call. */
int hobbit_commitment_is_half(const hobbit_commitment *c);

/* hobbit_aggregate over a real polynomial: d_aggr[j] = sum_i h_beta[i] * d_poly[i * (N / K) + j], products of F_{p^2} by F_p.  Any K > 0. */
int hobbit_aggregate_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_F *h_beta, int K, hobbit_F *d_aggr);

/* hobbit_open_standard for a real polynomial and its commitment (half or full): hobbit_aggregate_real, then the opening as it runs from an
 * aggregate; replies and paths come from the commitment.  Same outputs, same libc draws in the same order. */
int hobbit_open_standard_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_open_out *out);

/* generate_randomness(n) drawn on the device as reals: d_out[j] = the real part of element j (img is 0 in that stream), 8 bytes per value.
 * The process generator moves as hobbit_generate_randomness_dev moves it. */
int hobbit_generate_randomness_real_dev(hobbit_ctx *ctx, size_t n, uint64_t *d_out);

#ifdef __cplusplus
}
#endif
#endif
