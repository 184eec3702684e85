/* hobbit_elastic_real.h -- a header of libhobbit_hip.so beside hobbit_real.h: Elastic_PC, the streaming commitment, on streams whose values lie in
 * the BASE field F_p, p = 2^61 - 1 (the default streams of read_stream_PC and read_stream, the witness, wiring and trace streams of the circuit prover).
 *
 * A real chunk is `const uint64_t *`: B canonical values < p, 8 bytes each, 16-byte aligned.  conj(w) = w^p = 1/w for every root of unity of 2-power
 * order (the order divides p + 1 = 2^61), which gives three exact identities ("Elastic_PC on base-field streams"):
 *   rows               the L-point transform of a real row of L / 2 values, zero-padded, satisfies X[L - k] = conj(X[k]); X[0 .. L / 2] come from ONE
 *                      L / 2-point transform of the row read as L / 4 F elements and an unpacking pass (any L, not only 4096);
 *   columns, RS x exp  under base-field graph weights, T(r, cols - c) = conj(T(r, c));
 *   columns, RS x RS   the column code is a transform of rows2 = 2 trs points, so T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)).
 * A chunk's HALF tensor is columns 0 .. cols / 2, codeword-major, (cols / 2 + 1) x rows2 elements; half_ref of
 * csrc/hobbit_half.hpp is the one function that says where entry (r, c) of the full tensor lives in it and whether as a conjugate.
 * Everything here is bit-identical to the calls of hobbit_hip.h on the chunks widened to (x, 0) (hobbit_widen_real).
 *
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_ELASTIC_REAL_H
#define HOBBIT_ELASTIC_REAL_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The row code of real rows at any length L = 2^logL, 3 <= logL <= 16: `rows` rows of L / 2 reals (zero-padded to L points) -> rows x (L / 2 + 1) F,
 * row-major: X[0 .. L / 2] of hobbit_fft_any(logn = logL) on the widened, padded row.  logL = 12 is hobbit_fft_real_rows.  Asynchronous. */
int hobbit_fft_real_rows_any(hobbit_ctx *ctx, const uint64_t *d_reals, size_t rows, int logL, hobbit_F *d_out);

/* hobbit_elastic_begin for a stream of real chunks: the handle holds four half chunk tensors and the 4B running leaves.  B and trs powers of two,
 * row codes of 2^3 .. 2^16 points; linear_time = 0 (RS x RS) needs 2 trs <= 4096.  linear_time = 1 with finalized graphs that have a weight whose
 * img != 0 is HOBBIT_EINVAL before any launch (the column identity needs base-field weights); graphs for trs > 13 that are not finalized are
 * HOBBIT_ESTATE.  hobbit_elastic_finish and hobbit_elastic_free serve the handle as they serve hobbit_elastic_begin's. */
int hobbit_elastic_begin_real(hobbit_ctx *ctx, size_t B, int trs, int linear_time, int gcc_arg_order, hobbit_elastic **out);
/* hobbit_elastic_push of a real chunk (B values).  HOBBIT_ESTATE on a handle of hobbit_elastic_begin, as hobbit_elastic_push and
 * hobbit_elastic_push_inner are on a handle of hobbit_elastic_begin_real.  Asynchronous. */
int hobbit_elastic_push_real(hobbit_ctx *ctx, hobbit_elastic *e, const uint64_t *d_chunk);
/* Device bytes a streaming-commit handle (of either kind) holds: its four chunk tensors and the running leaves, as allocated. */
size_t hobbit_elastic_device_bytes(const hobbit_elastic *e);

/* The two passes of hobbit_elastic_open (hobbit_elastic_open_begin: option 1, hobbit_elastic_open_begin_lin: option 2, row codes of at most 2^16
 * points) on real chunks; begin, aggregate_finish, dims, finish and free are those of hobbit_hip.h.  Within one pass every chunk comes through the
 * same form, F or real: HOBBIT_ESTATE otherwise.  Asynchronous. */
int hobbit_elastic_open_aggregate_push_real(hobbit_ctx *ctx, hobbit_elastic_open *e, const uint64_t *d_chunk);
int hobbit_elastic_open_reply_push_real(hobbit_ctx *ctx, hobbit_elastic_open *e, const uint64_t *d_chunk);

#ifdef __cplusplus
}
#endif
#endif
