/* hobbit_longcodes.h -- a header of libhobbit_hip.so beside hobbit_brakingbase.h: the Braking base baseline (hobbit_brakingbase.h) at rows longer than 2^20, for
 * `./pigeon 28 5 128` of the reference's PC_tests.sh (trs = N / K = 2^21).
 *
 * hobbit_brakingbase_shape / _commit / _open keep their cap of 2^20 and their messages; the three calls here are the same bodies with the cap
 * at 2^21.  They take and make the same hobbit_brakingbase objects, read by the same accessors (hobbit_brakingbase_dims, _root, _levels,
 * _tensor, _matrix_dev, _levels_dev, _free).  Beneath them, in place: hobbit_graph_finalize, hobbit_encode_interleaved and
 * hobbit_prove_linear_code take n = 2^21; hobbit_parity_commit[_device] / hobbit_parity_shape / hobbit_parity_open take n = 2^21
 * (P = 2^26: a witness of 2^29 and encoded rows of 2^30 elements); hobbit_shockwave_prove routes aggregates wider than 2^24 (to 2^26) to the
 * table-free out-of-domain step of hobbit_whir_prove_any (hobbit_whir.h).
 *
 * Not served: trs = 2^22 (`./pigeon 28 5 64`).  There the parity matrix' encoded rows hold 2^31 elements; that size has not been run, so the
 * shape is refused rather than shipped unverified.
 *
 * Device memory at trs = 2^21, from the allocations' sizes: about 35 GiB for the parity commitment made inside the opening and about 60 GiB
 * of opening scratch and workspaces, which the context keeps.  The long calls ask hipMemGetInfo first and return HOBBIT_ENOMEM, before any
 * libc draw, allocation or launch, when that much is not free; so do hobbit_parity_commit[_device] and hobbit_parity_open past P = 2^25.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_LONGCODES_H
#define HOBBIT_LONGCODES_H
#include "hobbit_brakingbase.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hobbit_brakingbase_shape with 128 <= trs <= 2^21: every shape that call serves, and (2^28, 128), (2^23, 4), ...  Host only; trs may be NULL. */
int hobbit_brakingbase_shape_any(size_t N, size_t K, size_t *trs);

/* hobbit_brakingbase_commit at the shapes of hobbit_brakingbase_shape_any: same arguments, same object, same bits where both serve the shape.
 * Asynchronous on the context's stream; draws nothing from libc.  A refused shape is HOBBIT_EINVAL before any allocation or launch. */
int hobbit_brakingbase_commit_any(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, size_t K, int left_left_quirk, hobbit_brakingbase **out);

/* hobbit_brakingbase_open for a commitment of either commit: same arguments, outputs, libc draws and stages, returned synchronised.
 * (hobbit_brakingbase_open itself refuses a commitment with trs above 2^20.) */
int hobbit_brakingbase_open_any(hobbit_ctx *ctx, const hobbit_brakingbase *c, const hobbit_F *h_x, hobbit_brakingbase_open_out *out);

#ifdef __cplusplus
}
#endif
#endif
