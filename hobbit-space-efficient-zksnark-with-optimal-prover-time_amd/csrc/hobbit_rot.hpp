// The rotated message half of a commitment's tensor (hobbit_commitment::msg_rot).
//
// The tensor is codeword-major, [chunk][col][2 trs], so the column pitch is 2 trs 16 B = 128 KiB at trs = 4096 and a fixed row of all
// 4096 columns lies on one offset modulo that pitch.  A row FFT that stores the tensor itself writes exactly that pattern, 4096 stores per
// row onto a few memory channels (experiments (iv)(b) and (iv)(d)).  In a rotated tensor column c keeps its base and
// its pitch, but its message rows [0, trs) are rotated inside their own ring of trs elements:
//
//     row r < trs of column c lives at element (r + MSG_ROT_ELEMS c) mod trs of the column,   rows >= trs (the parity half) stay put.
//
// MSG_ROT_BYTES is a multiple of 128, so the eight rows of a 128-byte line and the four rows of a 64-byte leaf group stay contiguous and
// aligned, and for a fixed row the columns walk through every line of the ring.  128 B is the measured choice ((iv)(d): 128 B, 256 B,
// 512 B, 1 KiB and 4 KiB give 5.15 / 5.24 / 5.28 / 5.56 / 5.75 ms for the row FFT at 2^28 against 9.76 ms unrotated).
//
// Every reader and the one writer of a commitment's message half go through msg_rot_row, host and device alike.  rot_mask is
// hobbit_commitment::msg_rot: trs - 1 for a rotated tensor, 0 for a linear one (then msg_rot_row is the identity).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HB_ROT_HD __host__ __device__ __forceinline__
#else
#define HB_ROT_HD inline
#endif

namespace hobbit {

constexpr uint32_t MSG_ROT_BYTES = 128;
constexpr uint32_t MSG_ROT_ELEMS = MSG_ROT_BYTES / 16;
static_assert(MSG_ROT_BYTES % 128 == 0, "line groups of eight rows must stay whole");

// where row r of column c lives inside the column (in elements); c may be the column's index in the chunk or in the whole batch of chunks:
// the rotation has period trs / MSG_ROT_ELEMS in c, which divides the row length of every tensor that is rotated
HB_ROT_HD uint32_t msg_rot_elems(uint32_t c, uint32_t rot_mask) { return (MSG_ROT_ELEMS * c) & rot_mask; }      // column c's rotation, in elements
HB_ROT_HD uint32_t msg_rot_at(uint32_t r, uint32_t rot, uint32_t rot_mask) { return (r + rot) & rot_mask; }            // r <= rot_mask, rot = msg_rot_elems(c)
HB_ROT_HD uint32_t msg_rot_row(uint32_t r, uint32_t c, uint32_t rot_mask) { return r <= rot_mask ? msg_rot_at(r, msg_rot_elems(c, rot_mask), rot_mask) : r; }
// the inverse: which row the element at position p of column c holds
HB_ROT_HD uint32_t msg_unrot_row(uint32_t p, uint32_t c, uint32_t rot_mask) { return p <= rot_mask ? ((p - MSG_ROT_ELEMS * c) & rot_mask) : p; }

}  // namespace hobbit
