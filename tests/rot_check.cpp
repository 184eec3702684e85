// Stand-alone check of csrc/hobbit_rot.hpp (the index of a commitment's rotated message half), built by tests/test_tensor_rotation_cpu.py
// with the address and undefined-behaviour sanitizers: the same inline functions the kernels and the host call.
// Prints "<check> <count>" lines and exits 0, or names the first failure and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hobbit_rot.hpp"

using namespace hobbit;

static int fail(const char *what, uint32_t r, uint32_t c) { std::printf("FAIL %s r=%u c=%u\n", what, r, c); return 1; }

int main(int argc, char **argv) {
    const uint32_t trs = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096u, cols = 4096, mask = trs - 1;
    if (trs < 8 || (trs & mask)) return fail("trs must be a power of two >= 8", trs, 0);
    std::printf("S_bytes %u\n", MSG_ROT_BYTES);
    // (1) for every column (r -> place) is a bijection of the ring, un-rotate o rotate is the identity, and the parity half does not move
    std::vector<unsigned char> seen(trs);
    unsigned long long checked = 0;
    for (uint32_t c = 0; c < cols; c++) {
        std::fill(seen.begin(), seen.end(), 0);
        for (uint32_t r = 0; r < trs; r++) {
            const uint32_t p = msg_rot_row(r, c, mask);
            if (p >= trs) return fail("place outside the ring", r, c);
            if (seen[p]++) return fail("two rows on one place", r, c);
            if (msg_unrot_row(p, c, mask) != r) return fail("unrotate o rotate is not the identity", r, c);
            if (msg_rot_row(msg_unrot_row(r, c, mask), c, mask) != r) return fail("rotate o unrotate is not the identity", r, c);
            checked++;
        }
        for (uint32_t r = trs; r < 2 * trs; r += 37)
            if (msg_rot_row(r, c, mask) != r || msg_unrot_row(r, c, mask) != r) return fail("a parity row moved", r, c);
    }
    std::printf("bijection %llu\n", checked);
    // (2) four-row leaf groups (64 B) and eight-row line groups (128 B) stay contiguous and aligned
    unsigned long long groups = 0;
    for (uint32_t c = 0; c < cols; c++)
        for (uint32_t r = 0; r < trs; r += 4) {
            const uint32_t p = msg_rot_row(r, c, mask);
            if (p % 4) return fail("leaf group not aligned", r, c);
            for (uint32_t k = 1; k < 4; k++) if (msg_rot_row(r + k, c, mask) != p + k) return fail("leaf group not contiguous", r + k, c);
            if (r % 8 == 0) {
                if (p % 8) return fail("line group not aligned", r, c);
                for (uint32_t k = 4; k < 8; k++) if (msg_rot_row(r + k, c, mask) != p + k) return fail("line group not contiguous", r + k, c);
            }
            groups++;
        }
    std::printf("groups %llu\n", groups);
    // (3) over all columns a fixed row covers the ring evenly: every 128-byte line of the ring gets the same number of columns
    const uint32_t lines = trs / 8;
    std::vector<uint32_t> hist(lines);
    for (uint32_t r = 0; r < trs; r++) {
        std::fill(hist.begin(), hist.end(), 0u);
        for (uint32_t c = 0; c < cols; c++) hist[msg_rot_row(r, c, mask) / 8]++;
        for (uint32_t l = 0; l < lines; l++) if (hist[l] != cols / lines) return fail("a row does not cover the ring evenly", r, l);
    }
    std::printf("coverage %u\n", cols / lines);
    // (4) a linear tensor (mask 0): the identity on every row
    for (uint32_t c = 0; c < cols; c += 5)
        for (uint32_t r = 0; r < 2 * trs; r++)
            if (msg_rot_row(r, c, 0) != r || msg_unrot_row(r, c, 0) != r) return fail("mask 0 is not the identity", r, c);
    std::printf("linear ok\n");
    return 0;
}
