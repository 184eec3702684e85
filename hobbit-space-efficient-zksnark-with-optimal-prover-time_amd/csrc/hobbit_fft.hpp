// hobbit_fft.hpp -- the FFT module's whole surface (hobbit_fft.hip: kernels, twiddle tables, dispatch).  Same DFT as the reference's _fft
// (src/utils.cpp:605-673), natural order in and out, bit-exact by exactness of F_{p^2}.
#pragma once
#include "hobbit_ctx.hpp"

namespace hobbit {
namespace fft {

// The factor every result is multiplied by on the way out.  The default is the direction's own: none forward, 1/len inverse (src/utils.cpp:663-671).
struct Scale {
    int on = -1; F by = fmake(1);                       // on: -1 the direction's own, 0 none, 1 `by`
    static Scale none() { Scale s; s.on = 0; return s; }
};

// Rows of 2^logn <= 4096 points, row (g, r) of `groups` x `rows_per_group` at src + g src_gs + r src_ld (src_len elements, the rest of the transform
// length zero) -> dst + g dst_gs + r dst_ld, element stride dst_es (the tensor code writes its codeword-major layout this way).
int rows(hobbit_ctx *ctx, const F *src, size_t src_ld, uint32_t src_len, F *dst, size_t dst_ld, size_t dst_es, int logn, bool inverse, uint32_t groups,
         uint32_t rows_per_group, size_t src_gs, size_t dst_gs, Scale out = Scale());
// Every length up to 2^28: rows of src_len (the full length, or forward its zero-padded half) elements, src_ld apart -> contiguous rows of dst.
// 2^13 .. 2^24 run as two factors, 2^25 .. 2^28 as three; src may equal dst (from 2^25: full contiguous rows only).
int any_rows(hobbit_ctx *ctx, const F *src, size_t src_ld, size_t src_len, F *dst, int logn, bool inverse, size_t batch);
// The 4096-point row code of a tensor code (messages of 2048 elements, zero-padded), addressed like rows().  rot_mask (hobbit_rot.hpp): a
// commitment's rotated message half -- dst_ld == 1, row r of column c at its rotated place.
int rowcode_4096(hobbit_ctx *ctx, const F *src, size_t src_ld, F *dst, size_t dst_ld, size_t dst_es, uint32_t groups, uint32_t rows_per_group, size_t src_gs,
                 size_t dst_gs, uint32_t rot_mask = 0);
// The 4096-point row code of `nrows` base-field rows of 2048 reals (include/hobbit_real.h), columns 0 .. 2048.  tensor: rows (chunk, r) of K chunks of
// trs rows, the first of them row 0 of chunk chunk0, into a commitment's half tensor (hobbit_half.hpp), rotated by rot_mask; otherwise row-major,
// 2049 elements per row.
int rowcode_real4096(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, F *dst, bool tensor, uint32_t trs, uint32_t K, uint32_t rot_mask, uint32_t chunk0);
// The row code of `nrows` base-field rows of L / 2 reals, L = 2^logL, 3 <= logL <= 16 (include/hobbit_elastic_real.h), columns 0 .. L / 2: rowcode_real4096
// for logL = 12, otherwise the packed L / 2-point transform through any_rows (into workspace5) and k_real_unpack.  tensor: the nrows == trs rows of one
// chunk into the chunk's half tensor (hobbit_half.hpp: (L / 2 + 1) x 2 trs, codeword-major); otherwise row-major, L / 2 + 1 elements per row.
int real_rows_any(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst, bool tensor, uint32_t trs);
// The same row code at 3 <= logL <= 20 (include/hobbit_real_rs.h), row-major: above 2^16 the packed transform is the long one; the twiddle w^k of order L
// is read from the ROOTS table of that length.
int real_rows_len(hobbit_ctx *ctx, const uint64_t *src, size_t nrows, int logL, F *dst);
// The row code of `nchunks` whole chunks of trs base-field rows (2^(logL-1) reals each, 3 <= logL <= 20), the first of them chunk chunk0 of K, into a
// COMMITMENT's half tensor (hobbit_half.hpp: main block and strip), unrotated: rowcode_real4096 for logL = 12, otherwise the packed transform of all
// nchunks trs rows at once (workspace5) and k_real_unpack_half.
int rowcode_real_half(hobbit_ctx *ctx, const uint64_t *src, int logL, F *dst, uint32_t trs, uint32_t K, uint32_t nchunks, uint32_t chunk0);
// The 2^13 .. 2^15-point row code (Elastic_PC opt 2: 32768) of `nrows` contiguous messages of 2^(logc-1) elements: R = 2^(logc-12) strided FFT-4096 per
// row into Y, then the twiddles and the R-point combine into the row-major rm (both nrows 2^logc elements).
int rowcode_combine(hobbit_ctx *ctx, const F *msg, int logc, uint32_t nrows, F *Y, F *rm);
// w^k, k < 2^(logn-1), w = the order-2^logn root of unity or its inverse (phi_g reads them)
int roots(hobbit_ctx *ctx, int logn, bool inverse, const F **out);

}  // namespace fft

// Row-major (rows x cols, row stride in_ld / cols) -> codeword-major (cols x ld_out), `groups` matrices in_gs / out_gs apart
int launch_transpose_ld(hobbit_ctx *ctx, const F *in, size_t in_gs, size_t in_ld, uint32_t rows, uint32_t cols, F *out, size_t out_gs, size_t ld_out,
                        uint32_t groups);
int launch_transpose(hobbit_ctx *ctx, const F *in, size_t in_gs, uint32_t rows, uint32_t cols, F *out, size_t out_gs, size_t ld_out, uint32_t groups);
}  // namespace hobbit
