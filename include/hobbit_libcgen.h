/* hobbit_libcgen.h -- a header of libhobbit_hip.so beside hobbit_hip.h: the libc random stream drawn on the device.
 *
 * Every challenge of the reference that is not a transcript hash, its polynomial (generate_randomness) and its expander graphs
 * (expander_init_store) are rand() / random() calls on the process-wide glibc generator, one call per value.  glibc's default generator
 * (TYPE_3) is the additive recurrence r_i = r_{i-3} + r_{i-31} mod 2^32, a draw returning r_i >> 1, shared by rand() and random().  A WINDOW
 * is its 31 words r_{i-31} .. r_{i-1}, oldest first; DRAW j of a window is the value the j-th call from that state returns.  The recurrence
 * is linear, so the window k draws ahead costs O(log k) products of 31 x 31 words, and any number of device lanes can each start at their own
 * offset.  The calls here return the values the host loops would have returned and leave the process generator where those loops would have
 * left it; nothing that existed before them changes what it returns or where it leaves the generator.
 *
 * A generator whose state is not TYPE_3 (the caller ran initstate with a buffer outside 128..255 bytes) is refused with HOBBIT_ESTATE by every
 * call that reads or writes the process generator, and is left exactly as it was.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_LIBCGEN_H
#define HOBBIT_LIBCGEN_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- host only (no context, no device) ---- */
/* the process generator as a window; the generator is not disturbed */
int hobbit_libc_window(uint32_t w[31]);
/* make the process generator continue from window w (on a state block the library owns, as after an initstate of the caller's own) */
int hobbit_libc_set_window(const uint32_t w[31]);
/* move the process generator k draws ahead without drawing: the next rand() returns what it would have returned after k calls */
int hobbit_libc_advance(uint64_t k);
/* the window k draws ahead of w: a pure function (out may alias w) */
void hobbit_libc_jump(const uint32_t w[31], uint64_t k, uint32_t out[31]);

/* the raw-draw kernel's shape: draws one lane runs through sequentially, draws one workgroup covers (the sizes at which its paths change) */
void hobbit_libc_draws_shape(size_t *run_length, size_t *workgroup_span);

/* ---- device.  Pure functions of their arguments: the process generator is neither read nor moved.  Queued on the context's stream. ---- */
/* d_out[j] = draw first + j of window w, j < n */
int hobbit_libc_draws_dev(hobbit_ctx *ctx, const uint32_t w[31], uint64_t first, size_t n, uint32_t *d_out);
/* One expander level as generate_random_expander_store(L, R, degree) draws it from draw `first` of w on: edge e = i * degree + j has
 * d_nbr[e] = (draw first + 2e) mod R and d_w[e] = F(draw first + 2e + 1) -- the arrays hobbit_graph_upload takes.  0 < R < 2^31. */
int hobbit_libc_graph_level_dev(hobbit_ctx *ctx, const uint32_t w[31], uint64_t first, long long L, long long R, int degree, long long *d_nbr, hobbit_F *d_w);

/* ---- device, on the process generator ---- */
/* d_out = what hobbit_generate_randomness(n, .) would return at this point of the process; the process generator is left n + ceil(n / 100)
 * draws further on return, while the fill is queued on the context's stream like hobbit_fill_splitmix. */
int hobbit_generate_randomness_dev(hobbit_ctx *ctx, size_t n, hobbit_F *d_out);
/* expander_init_store(n): hobbit_graph_reset, every level drawn on the device in the reference's order (C[0], C[1], ..., D[last], ..., D[0]) from
 * the process generator's position, read back into the context's graph store, hobbit_graph_finalize(n).  The process generator is left
 * 2 * (total edges) draws further.  HOBBIT_ESTATE comes before anything is changed.  Returned synchronised. */
int hobbit_graph_draw(hobbit_ctx *ctx, long long n, long long *codeword_len);
/* One level of the context's graph store (hobbit_graph_upload / hobbit_graph_draw): dimensions and HOST pointers to its neighbour and weight
 * arrays, valid until the next hobbit_graph_reset / _upload / _draw.  Any output may be NULL.  HOBBIT_ESTATE when the level is not there. */
int hobbit_graph_level_host(hobbit_ctx *ctx, int dep, int kind, long long *L, long long *R, int *degree, const long long **h_nbr, const hobbit_F **h_w);

#ifdef __cplusplus
}
#endif
#endif
