// The half form of a commitment's tensor (hobbit_commitment::half; include/hobbit_real.h).
//
// A commitment to a base-field polynomial under base-field expander weights has, in every chunk, column cols - c equal to the entry-wise
// conjugate of column c (parity half included), and columns 0 and cols / 2 equal to their own conjugates.  A half tensor stores columns
// 0 .. cols / 2 of every chunk and nothing else, as ONE batch of K hc + K codeword-major columns of 2 trs elements, hc = cols / 2:
//
//     main block   [K][hc][2 trs]    column c < hc of chunk i is batch column i hc + c
//     strip        [K][2 trs]        column hc of chunk i is batch column K hc + i
//
// The encode runs over the batch as over any other; a rotated message half (hobbit_rot.hpp) is rotated by the BATCH column, whose period
// trs / MSG_ROT_ELEMS divides hc wherever a tensor is rotated.  rows_valid and msg_rot mean what they mean for a full tensor.
// Every reader and the one writer of a half tensor go through half_col: the row FFT (k_fft_real4096), the leaf chain, the gather, the row read
// and the mirror that materialises the full tensor.  A reader answers column c > hc as the conjugate of column cols - c.
#pragma once
#include "hobbit_field.hpp"
#include "hobbit_rot.hpp"

namespace hobbit {

// the column whose memory answers column c, and whether the answer is its conjugate
HB_ROT_HD uint32_t half_src_col(uint32_t c, uint32_t cols) { return c <= cols / 2 ? c : cols - c; }
HB_ROT_HD bool half_is_conj(uint32_t c, uint32_t cols) { return c > cols / 2; }
// batch column of stored column sc <= cols / 2 of chunk i (K chunks)
HB_ROT_HD size_t half_col(uint32_t i, uint32_t sc, uint32_t cols, uint32_t K) {
    const uint32_t hc = cols / 2;
    return sc < hc ? (size_t)i * hc + sc : (size_t)K * hc + i;
}
HB_ROT_HD size_t half_ncols(uint32_t cols, uint32_t K) { return (size_t)K * (cols / 2) + K; }
// element offset of row r of stored column sc of chunk i
HB_ROT_HD size_t half_at(uint32_t i, uint32_t sc, uint32_t r, uint32_t cols, uint32_t K, uint32_t rows2, uint32_t rot_mask) {
    const size_t g = half_col(i, sc, cols, K);
    return g * rows2 + msg_rot_row(r, (uint32_t)g, rot_mask);
}
// One chunk's half tensor of the streaming commit (include/hobbit_elastic_real.h): columns 0 .. cols / 2, codeword-major, (cols / 2 + 1) x rows2,
// the layout above at K = 1, unrotated.  half_ref answers, for entry (r, c) of the full chunk tensor, which stored entry holds it and whether
// as its conjugate.  RS x expander (linear_time): T(r, cols - c) = conj(T(r, c)).  RS x RS: the column code is a transform of rows2 points, so
// T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)) -- the conjugate, with the row index negated.
struct HalfRef { uint32_t row, col; bool conj; };
HB_ROT_HD HalfRef half_ref(uint32_t r, uint32_t c, uint32_t cols, uint32_t rows2, int linear_time) {
    if (!half_is_conj(c, cols)) return HalfRef{r, c, false};
    return HalfRef{linear_time || !r ? r : rows2 - r, cols - c, true};
}
// the row of the full entry in column cols - sc that stored entry (row, sc) answers as its conjugate (0 < sc < cols / 2): half_ref's inverse
HB_ROT_HD uint32_t half_mirror_row(uint32_t row, uint32_t rows2, int linear_time) { return linear_time || !row ? row : rows2 - row; }
// element offset of stored entry (row, sc) in a chunk's half tensor
HB_ROT_HD size_t half_chunk_at(uint32_t row, uint32_t sc, uint32_t rows2) { return (size_t)sc * rows2 + row; }
// conj(a + bi) = a - bi, canonical in and out
HB_HD F fconj(const F &a) { return fmake(a.re, a.im ? P61 - a.im : 0); }

}  // namespace hobbit
