/* hobbit_whir.h -- third header of libhobbit_hip.so: WHIR proofs of every length hobbit_whir_commit serves.
 *
 * hobbit_whir_prove (hobbit_hip.h) stops at N = 2^24: its out-of-domain step materialises one full eq table per point, 2 x 100 x N/16
 * elements of scratch.  The calls here run the same proof, _whir_prove (src/Virgo.cpp:519-686), with that step computed from the two
 * halves of every table, and reach N = 2^26: the reference's standalone WHIR baseline (test_PC's last branch, src/Our_PC.cpp:843-859) and
 * the widths the parity opening of the long codes asks for.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_WHIR_H
#define HOBBIT_WHIR_H
#include "hobbit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The out-of-domain step of one _whir_prove iteration (src/Virgo.cpp:613-633) for R points z_i in F^v over cur = 2^v coefficients:
 *     d_y[i]   = <eq(z_i), d_poly>                         (R F, written)
 *     d_beta  += sum_i h_pw[i] * eq(z_i)                   (cur F, updated in place)
 * with eq(z) = precompute_beta(z): z[0] sits on the least significant bit of the index.  No table of cur entries is built: with
 * vl = min(v, 4), eq(z)[h * 2^vl + l] = eq(z[vl..v))[h] * eq(z[0..vl))[l], the R low tables (2^vl entries) sit in LDS, the R high tables
 * (2^(v - vl) entries) in the context's workspace, and d_poly and d_beta cross memory once each.  The field is exact, so the result has
 * the bits of the materialised form.
 * h_z: R x v F, point-major; h_pw: R F.  1 <= v <= 26, 1 <= R <= 128 (else HOBBIT_EINVAL, nothing queued).
 * Asynchronous; h_z and h_pw are consumed before the call returns.  Workspace: 2048 + 2 R 2^(v - vl) + 1024 R + (R (v + vl + 1)) F. */
int hobbit_whir_ood(hobbit_ctx *ctx, const hobbit_F *d_poly, hobbit_F *d_beta, int v, const hobbit_F *h_z, const hobbit_F *h_pw, int R, hobbit_F *d_y);

/* hobbit_whir_prove for every power of two 2^9 <= N <= 2^26: same arguments, same hobbit_whir_out, the same libc draws in the same order,
 * and the same bits wherever hobbit_whir_prove serves the shape.  One path at every size: the out-of-domain step is hobbit_whir_ood's, the
 * FRI layers of 2^25 and 2^26 points go through the any-length transform.  2^25 and 2^26 are the first sizes with six iterations
 * (fri_roots: 6 x 32 B, qpoly: 24 x 3 F, up to 160 queries and 123 200 path bytes).
 * A refused N (HOBBIT_EINVAL) draws nothing from libc and launches nothing.
 * Scratch (workspace4, F elements): 4 N (left to a hobbit_whir_commit of the same polynomial) + 2 N (polynomial, beta)
 *   + 2048 + 200 max(N / 256, 1) + 100 * 1024 (out-of-domain step: low tables, two high-table buffers, per-workgroup partial sums)
 *   + N (FRI scratch) + 3 N (two kept layers with their trees) + about 34 000 (staging, results, query answers).
 * Nothing grows with R * cur: 10.8 N against hobbit_whir_prove's 22.5 N. */
int hobbit_whir_prove_any(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_F *d_com, const uint8_t *d_com_levels, const hobbit_F *h_x, hobbit_whir_out *out);

#ifdef __cplusplus
}
#endif
#endif
