// hobbit_kernels.hpp -- launcher prototypes (definitions in hobbit_kernels.hip)
#pragma once
#include "hobbit_ctx.hpp"
#include "hobbit_rot.hpp"
#include "hobbit_half.hpp"

namespace hobbit {
// The longest code: hobbit_graph_finalize, the rows-innermost encode, hobbit_parity_commit[_device] / hobbit_parity_open and the long forms of
// include/hobbit_longcodes.h stop at n = 2^CODE_MAX_LOG.  At 2^21 the parity matrix' padded list has P = 2^26 entries and its encoded rows
// 2^30 elements; 2^22 would put an element index past 2^31 and is not served (DESIGN.md section 4 "Codes of 2^21").
constexpr int CODE_MAX_LOG = 21;
// HOBBIT_ENOMEM unless the device has `bytes` free right now (hipMemGetInfo): asked before the large allocations of the long codes, on
// machines whose memory other processes share, and before any libc draw of the call.  `what` names the caller in the message.
int need_device_bytes(hobbit_ctx *ctx, size_t bytes, const char *what);
// The parity matrix past P = 2^25 (n = 2^21), in device bytes.  A commitment: its five buffers (480 P + 32 S), the sort's keys, places and
// scratch and the three transform workspaces of hobbit_shockwave_commit's 16 rows of P points (80 P).  An opening: its own scratch (320 P),
// the multiplication tree's arena over 4 P (256 P), P4's ping-pong tables over 8 P (192 P), shockwave_prove(C_p) at width P / 2 with its
// nested WHIR proof (152 P) and prove_fft's tables (32 P) -- workspaces the context keeps.  Sums of the allocations' sizes, not measurements.
inline bool parity_is_long(size_t P) { return P > ((size_t)1 << 25); }
inline size_t parity_commit_bytes(size_t P, size_t S) { return 560 * P + 32 * S; }
inline size_t parity_open_bytes(size_t P) { return 952 * P; }
// plans built on first use (hobbit_capi.hip): the tiled steps of a long code, the CSR steps of the rows-innermost encode
int ensure_tiled(hobbit_ctx *ctx);
int ensure_ilv(hobbit_ctx *ctx);
// the access lists of the parity matrix: their segment table from the finalized plan (host only), and the forward form on the device
int parity_segments(hobbit_ctx *ctx, std::vector<ParitySeg> &segs, size_t *m);
int ensure_fwd(hobbit_ctx *ctx);
int launch_encode_ilv(hobbit_ctx *ctx, const F *src, F *dst, uint32_t rows);
// the rows-innermost encode in place on a 2n x ld matrix over its first `width` columns, strip-major (strip: columns per strip, 0 = plain order)
int launch_encode_ilv_ld(hobbit_ctx *ctx, F *mat, uint32_t width, size_t ld, uint32_t strip);
int launch_zero_rect(hobbit_ctx *ctx, F *mat, size_t ld, size_t row_lo, size_t nrows, size_t col_lo, size_t ncols);
// the body of hobbit_brakedown_commit for `rows` messages of B elements (hobbit_capi.hip); the caller has checked the shape and the graphs
int brakedown_commit_shape(hobbit_ctx *ctx, const F *d_poly, size_t B, uint32_t rows, int left_left_quirk, hobbit_brakedown **out);
int launch_brakedown_digests(hobbit_ctx *ctx, const F *mat, uint32_t rows, size_t ncols, size_t nz, int quirk, uint8_t *out);
int launch_brakedown_aggr(hobbit_ctx *ctx, const F *mat, uint32_t rows, size_t B, const F *beta, const F *r, F *aggr_beta, F *aggr_r);
int launch_brakedown_reply(hobbit_ctx *ctx, const F *mat, uint32_t rows, const uint32_t *d_I, size_t nq, F *reply);
int launch_bds_put(hobbit_ctx *ctx, const F *chunk, size_t B, uint32_t slot, F *mat);
int launch_bds_leaf(hobbit_ctx *ctx, const F *mat, size_t len, size_t W, int shift, uint8_t *state);
int launch_bds_aggr(hobbit_ctx *ctx, const F *mat, size_t B, const F *beta, const F *rv, F *ab, F *ar);
int launch_bds_reply(hobbit_ctx *ctx, const F *mat, const uint32_t *d_I, size_t nq, size_t chunks, size_t first, F *reply);
int launch_f_binop(hobbit_ctx *ctx, int op, const F *a, const F *b, F *o, size_t n);
int launch_fill_splitmix(hobbit_ctx *ctx, F *o, size_t n, uint64_t seed);
int launch_u64_bias_fold(hobbit_ctx *ctx, uint64_t *w, size_t n, uint64_t bias, int fold);
int launch_elastic_leaf(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, uint8_t *state);
int launch_elastic_inner(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, uint8_t *out);
int launch_elastic_finish(hobbit_ctx *ctx, const uint8_t *state, uint32_t rows2, uint32_t cols, uint8_t *leaves);
// rot_mask (hobbit_rot.hpp): the message half of every column is rotated; served by the fat in-place form only (encode_reads_rotated)
int launch_encode(hobbit_ctx *ctx, const F *src, size_t ld_src, F *dst, size_t ld_dst, long long n, size_t batch, int write_msg, uint32_t rot_mask = 0);
// whether the in-place encode of the finalized code for n reads its message through k_enc_fat's loader, the one form that knows the rotation
bool encode_reads_rotated(const hobbit_ctx *ctx, long long n);
int launch_blake3_64(hobbit_ctx *ctx, const uint8_t *in, uint8_t *out, size_t n);
int launch_hash_md(hobbit_ctx *ctx, const F *xyzw, const uint8_t *prev, uint8_t *out, size_t n);
int launch_merkle_levels(hobbit_ctx *ctx, uint8_t *levels, size_t n, int quirk);
int launch_leaf_chain_relay(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, size_t g_begin, size_t g_count,
                            const uint8_t *state_in, uint8_t *state_out, uint8_t *leaves, uint32_t zero_rows_from, int leaves_inout = 0);
// the commit's chain: starts from the zero state, so the leaves of the groups at or past zero_rows_from are written as one host-computed constant
int launch_leaf_chain(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves, uint32_t zero_rows_from,
                      uint32_t rot_mask = 0);
int launch_inner_digests(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int nchunks, uint32_t cols, uint32_t half_trs, uint8_t *out);
int launch_chain_digests(hobbit_ctx *ctx, const uint8_t *digests, size_t stride_bytes, int K, size_t m, uint8_t *leaves);
int launch_merkle_paths(hobbit_ctx *ctx, const uint8_t *levels, size_t n, const uint64_t *d_pos, size_t nq, int depth, uint8_t *d_paths);
int launch_eq_table(hobbit_ctx *ctx, CHP h_r, int k, F *d_out);
int launch_aggregate(hobbit_ctx *ctx, const F *poly, size_t M, int K, CHP h_beta, F *aggr);
int launch_gather(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, uint32_t rows2, int K, const uint32_t *d_rows, const uint32_t *d_cols,
                  size_t nq, F *d_reply, uint32_t rows_valid, uint32_t rot_mask = 0);
int launch_zero_rows(hobbit_ctx *ctx, F *tensor, size_t ncols, uint32_t rows2, uint32_t rows_valid);
int launch_tensor_row(hobbit_ctx *ctx, const F *chunk, uint32_t rows2, uint32_t cols, uint32_t row, F *d_out, uint32_t rows_valid, uint32_t rot_mask = 0);
// a rotated message half made linear, in place: rows [0, rot_mask] of each of the ncols columns (hobbit_commitment_tensor_dev)
int launch_unrotate_msg(hobbit_ctx *ctx, F *tensor, size_t ncols, uint32_t rows2, uint32_t rot_mask);
// The half form of a commitment's tensor (hobbit_half.hpp): the leaf chain, the gather and the row read over columns 0 .. cols / 2 in memory, the
// mirror that materialises the full linear tensor [K][cols][rows2], and the real-polynomial forms of the widening copy and the aggregate
int launch_leaf_chain_half(hobbit_ctx *ctx, const F *tensor, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves, uint32_t zero_rows_from, uint32_t rot_mask);
// lin: the commitment's column code -- 1 RS x expander (column cols - c is the conjugate of column c, row for row), 0 RS x RS (of the negated row)
int launch_gather_half(hobbit_ctx *ctx, const F *tensor, uint32_t cols, uint32_t rows2, int K, const uint32_t *d_rows, const uint32_t *d_cols, size_t nq, F *d_reply,
                       uint32_t rows_valid, uint32_t rot_mask, int lin = 1);
int launch_tensor_row_half(hobbit_ctx *ctx, const F *tensor, uint32_t chunk, int K, uint32_t rows2, uint32_t cols, uint32_t row, F *d_out, uint32_t rows_valid,
                           uint32_t rot_mask, int lin = 1);
int launch_half_expand(hobbit_ctx *ctx, const F *tensor, F *full, uint32_t cols, int K, uint32_t rows2, uint32_t rows_valid, uint32_t rot_mask, int lin = 1);
// the leaf chain over an RS x RS half tensor (include/hobbit_real_rs.h): one thread per stored group, two leaves; half_trs = rows2 / 4 groups, a power of two
int launch_leaf_chain_half_rs(hobbit_ctx *ctx, const F *tensor, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves);
int launch_widen_real(hobbit_ctx *ctx, const uint64_t *x, F *o, size_t n);
int launch_aggregate_real(hobbit_ctx *ctx, const uint64_t *poly, size_t M, int K, CHP h_beta, F *aggr);
int launch_eval_fold(hobbit_ctx *ctx, const F *v, F *o, size_t L, F r);
int launch_eval_fold2(hobbit_ctx *ctx, const F *v, F *o, size_t L, F r0, F r1);
int launch_eval_tail(hobbit_ctx *ctx, const F *v, F *o, size_t n, int levels, const F *r);
int launch_csr_gather(hobbit_ctx *ctx, const uint32_t *rowptr, const uint32_t *idx, const F *w, const F *x, F *y, size_t rows);
int launch_phi_step(hobbit_ctx *ctx, F *g, size_t half, int m, F rx, const F *pm, int last_only);
int launch_phi_head(hobbit_ctx *ctx, F *g, int n, int h, CHP h_rx, F scale, const F *pm);
int launch_fold_rows(hobbit_ctx *ctx, const F *in, F *out, size_t out_rows, size_t cols, F r);
int launch_matvec_rows(hobbit_ctx *ctx, const F *Mx, size_t rows, size_t cols, const F *v, F *out);
int launch_vecmat(hobbit_ctx *ctx, const F *Mx, size_t rows, size_t cols, const F *v, F *out);
int launch_gather_strided(hobbit_ctx *ctx, const F *src, const uint64_t *d_idx, size_t nq, uint32_t m, size_t bmul, size_t stride, F *out);
int launch_dot(hobbit_ctx *ctx, const F *a, const F *b, size_t n, F *part, F *out);
int launch_change_form_tail(hobbit_ctx *ctx, F *data, size_t n, uint32_t T);
int launch_scatter(hobbit_ctx *ctx, const uint64_t *idx, const F *val, size_t n, F *out);
int launch_axpy(hobbit_ctx *ctx, F *y, const F *x, F a, size_t n);
int launch_err_terms(hobbit_ctx *ctx, int kind, const F *const *tables, const int32_t *gate, size_t n, MHP h_K);
int launch_axpy_i32(hobbit_ctx *ctx, F *y, const int32_t *sel, F a, int one_minus, size_t n);
int launch_sc3_poly(hobbit_ctx *ctx, const F *s1, const F *s2, const F *s3, size_t L, F *part, F *coef);
int launch_fold3(hobbit_ctx *ctx, const F *s1, const F *s2, const F *s3, F *d1, F *d2, F *d3, size_t L, F r);
int launch_mul_layer(hobbit_ctx *ctx, const F *x, size_t n_out, F *in1, F *in2, F *tr);
int launch_fingerprint(hobbit_ctx *ctx, const F *addr, const F *value, const F *freq, F a, F b, F *out, size_t n);
int launch_col_digest(hobbit_ctx *ctx, const F *enc, size_t W, int k, int quirk, uint8_t *out);
int launch_change_form_level(hobbit_ctx *ctx, const F *in, F *out, size_t n, size_t S);
int launch_whir_round(hobbit_ctx *ctx, F *poly, F *beta, size_t L, F a, F *part, F *coef);
int launch_eq_step_batched(hobbit_ctx *ctx, const F *old, F *nw, size_t m, size_t ld, const F *z, int v, int level, int reps);
int launch_eq_head_batched(hobbit_ctx *ctx, F *out, size_t ld, const F *z, int v, int h, int reps);
// hobbit_whir.hip: the out-of-domain step from the two halves of every eq table (low half: WHIR_OOD_VL variables, in LDS)
static constexpr int WHIR_OOD_VL = 4;
size_t whir_ood_scratch_elems(int v, int R);
int launch_whir_ood(hobbit_ctx *ctx, const F *poly, F *beta, int v, const F *dz, const F *dzlo, const F *dpw, int R, F *scratch, F *d_y);
int launch_fill_F(hobbit_ctx *ctx, F *p, size_t stride, size_t n, F v);
int launch_sumcheck2(hobbit_ctx *ctx, const F *v1, const F *v2, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final);
int launch_sumcheck2_eq(hobbit_ctx *ctx, int T, CHP h_r1, CHP h_r2, CHP h_a, const F *v2, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final);
int launch_sumcheck2_sparse(hobbit_ctx *ctx, const F *v1, const uint64_t *d_idx, const F *d_val, size_t m, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final);
int launch_gate_lkp_sumcheck(hobbit_ctx *ctx, const F *const tabs[9], size_t n, CHP h_a, MHP h_rand, MHP h_sum, MHP h_poly, MHP h_r, MHP h_final, int *h_check);
int launch_lkp_prepare(hobbit_ctx *ctx, const int32_t *S, const F *L, const F *R, const F *O, int32_t *s2, int32_t *s3, F *blo, size_t n);
int launch_lkp_sel_fold(hobbit_ctx *ctx, const int32_t *S, F rnd, F *aL, F *aR, F *lkp, F *mul, size_t n);
int launch_gate_sumcheck(hobbit_ctx *ctx, const F *const tabs[6], size_t n, CHP h_a, MHP h_rand, MHP h_sum, MHP h_poly, MHP h_r, MHP h_final, int *h_check);
int launch_sumcheck3(hobbit_ctx *ctx, const F *v1, const F *v2, const F *v3, size_t n, F prev_r, MHP h_cpoly, MHP h_r, MHP h_vr, MHP h_final);
int launch_any_nonzero(hobbit_ctx *ctx, const F *v, size_t n, int *d_flag);
int launch_gather_cols(hobbit_ctx *ctx, const F *T, size_t ld, uint32_t nrows, const uint32_t *d_cols, uint32_t ncols, F *G, size_t ldG);
// the streaming commit and opening on base-field chunks (include/hobbit_elastic_real.h)
int launch_elastic_leaf_half(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, int lin, uint8_t *state);
int launch_gather_cols_half(hobbit_ctx *ctx, const F *T, uint32_t cols, uint32_t nrows, const uint32_t *d_cols, uint32_t ncols, F *G, size_t ldG);
int launch_axpy_real(hobbit_ctx *ctx, F *y, const uint64_t *x, F a, size_t n);
int launch_any_nonzero_real(hobbit_ctx *ctx, const uint64_t *v, size_t n, int *d_flag);
int launch_spread_cols(hobbit_ctx *ctx, const uint32_t *d_cols, const F *d_vals, uint32_t ncols, uint32_t nrows, size_t ld, F *out);
int launch_seg_prod(hobbit_ctx *ctx, const F *in, uint32_t seg, size_t n_out, F *out);
int launch_deinterleave(hobbit_ctx *ctx, const F *v, size_t n, F *a, F *b);
int launch_dot_gen(hobbit_ctx *ctx, const F *a, const F *b, size_t sb, const F *c, size_t n, F *part, F *out);
int launch_dot_i32(hobbit_ctx *ctx, const F *a, const int32_t *sel, int one_minus, size_t n, F *part, F *out);
int launch_i32_to_F(hobbit_ctx *ctx, const int32_t *sel, int one_minus, size_t n, F *y);
int launch_zero(hobbit_ctx *ctx, void *p, size_t bytes);
int launch_copy(hobbit_ctx *ctx, void *d, const void *s, size_t bytes);
}  // namespace hobbit
