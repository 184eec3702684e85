/* hobbit_real_rs.h -- a header of libhobbit_hip.so beside hobbit_real.h and hobbit_elastic_real.h: Our_PC under RS x RS (linear_time = 0: test_PC
 * option 1, the circuit polynomial of prove_circuit_standard) for polynomials whose coefficients lie in the BASE field F_p, p = 2^61 - 1.
 *
 * A real polynomial is `const uint64_t *`: N canonical values < p, 8 bytes each, 16-byte aligned.  Two exact identities of conj(a + bi) = a - bi
 * ("Base-field polynomials under RS x RS") halve the commitment:
 *   rows     the L-point transform of a real row of L / 2 values, zero-padded, satisfies X[L - k] = conj(X[k]); X[0 .. L / 2] come from ONE packed
 *            L / 2-point transform and an unpacking pass -- here at every L = 2^3 .. 2^20, where hobbit_fft_real_rows_any ends at 2^16;
 *   columns  the column code is a transform of rows2 = 2 trs points, so T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)): the conjugate, with the
 *            row index negated.
 * hobbit_commit_standard_real_rs therefore transforms and stores columns 0 .. cols / 2 of every chunk only: a HALF commitment
 * with lin = 0.  It is an ordinary hobbit_commitment for every accessor of hobbit_hip.h -- root, levels, paths, tensor_row, gather answer as the full
 * one does, bit for bit; hobbit_commitment_is_half is 1; hobbit_commitment_tensor_dev materialises the full linear tensor once -- and for
 * hobbit_open_standard_rs and hobbit_open_standard_rs_real.  Everything here is bit-identical to the calls of hobbit_hip.h on the polynomial widened
 * to (x, 0) (hobbit_widen_real).  hobbit_commit_standard_real(..., linear_time = 0) keeps refusing: this header is where RS x RS lives.
 *
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_REAL_RS_H
#define HOBBIT_REAL_RS_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The row code of real rows at any length L = 2^logL, 3 <= logL <= 20: `rows` rows of L / 2 reals (zero-padded to L points) -> rows x (L / 2 + 1) F,
 * row-major: X[0 .. L / 2] of hobbit_fft_any(logn = logL) on the widened, padded row.  The bits of hobbit_fft_real_rows_any where both apply; above
 * 2^16 the packed L / 2-point transform is the long one and the twiddle w^k of order L is read from the table of that length.  Asynchronous. */
int hobbit_fft_real_rows_len(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, int logL, hobbit_F *d_out);

/* hobbit_commit_standard(..., linear_time = 0) of a real polynomial, as a half commitment.  Shapes: K > 0 dividing N, N / K a power of two, trs >= 4 a
 * multiple of 4 with 2 trs a power of two <= 4096, and a row code of 8 <= 2 (N / K) / trs <= 2^20 points.  Everything else -- a null or not 16-byte
 * aligned polynomial included -- is HOBBIT_EINVAL with a message that says why, before any allocation or launch.  The expander graphs are not looked
 * at.  Asynchronous, like hobbit_commit_standard. */
int hobbit_commit_standard_real_rs(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, hobbit_commitment **out);
/* The same from (pageable) host memory: h_poly is streamed into d_poly (N * 8 bytes, the caller's) group by group under the commit's kernels, as
 * hobbit_commit_standard_host streams 16 bytes per coefficient. */
int hobbit_commit_standard_real_rs_host(hobbit_ctx *ctx, const uint64_t *h_poly, uint64_t *d_poly, size_t N, int K, int trs, hobbit_commitment **out);

/* hobbit_open_standard_rs for a real polynomial and its RS x RS commitment (half or full): hobbit_aggregate_real's kernel, then the opening as
 * hobbit_open_standard_rs runs it -- C_f, the draws, replies and paths out of the commitment, the RS prover.  Same outputs, same libc draws in the
 * same order.  An RS x expander commitment is HOBBIT_EINVAL, as it is for hobbit_open_standard_rs. */
int hobbit_open_standard_rs_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_elastic_open_out *out);

#ifdef __cplusplus
}
#endif
#endif
