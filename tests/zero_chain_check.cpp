// Stand-alone check of blake3_zero_group_leaf (csrc/hobbit_blake3.hpp), the constant leaf Z_K that the commit's launcher computes on the host
// and k_leaf_chain stores into the leaves of the all-zero groups: for K = 1, 2, 32 it must equal a plain loop
//     st = 0^32;  K times: st = H(H(0^64) | st)
// over a BLAKE3 compression written here straight from the specification (state in an array, the message permuted between rounds) -- nothing
// shared with the header's unrolled schedule.  Prints "K hex" per line for the caller to compare with its own references; exit status 1 on a
// mismatch.  tests/test_leaf_chain_zero_groups_cpu.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hobbit_blake3.hpp"

static uint32_t rotr(uint32_t x, int c) { return (x >> c) | (x << (32 - c)); }
static void g(uint32_t *v, int a, int b, int c, int d, uint32_t x, uint32_t y) {
    v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 12);
    v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 8);  v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 7);
}
// BLAKE3 of exactly 64 bytes to 32: one compression with the IV as chaining value, counter 0, block length 64, flags CHUNK_START | CHUNK_END | ROOT
static void plain_hash64(const uint8_t in[64], uint8_t out[32]) {
    static const uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    static const int PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    uint32_t m[16], v[16];
    for (int i = 0; i < 16; i++) m[i] = (uint32_t)in[4 * i] | (uint32_t)in[4 * i + 1] << 8 | (uint32_t)in[4 * i + 2] << 16 | (uint32_t)in[4 * i + 3] << 24;
    for (int i = 0; i < 8; i++) v[i] = IV[i];
    for (int i = 0; i < 4; i++) v[8 + i] = IV[i];
    v[12] = 0; v[13] = 0; v[14] = 64; v[15] = 1 | 2 | 8;
    for (int r = 0; r < 7; r++) {
        g(v, 0, 4, 8, 12, m[0], m[1]);   g(v, 1, 5, 9, 13, m[2], m[3]);   g(v, 2, 6, 10, 14, m[4], m[5]);   g(v, 3, 7, 11, 15, m[6], m[7]);
        g(v, 0, 5, 10, 15, m[8], m[9]);  g(v, 1, 6, 11, 12, m[10], m[11]); g(v, 2, 7, 8, 13, m[12], m[13]); g(v, 3, 4, 9, 14, m[14], m[15]);
        uint32_t t[16];
        for (int i = 0; i < 16; i++) t[i] = m[PERM[i]];
        memcpy(m, t, sizeof m);
    }
    for (int i = 0; i < 8; i++) {
        const uint32_t w = v[i] ^ v[i + 8];
        out[4 * i] = (uint8_t)w; out[4 * i + 1] = (uint8_t)(w >> 8); out[4 * i + 2] = (uint8_t)(w >> 16); out[4 * i + 3] = (uint8_t)(w >> 24);
    }
}

int main() {
    // the compression itself first: "abc..." test bytes through both
    {
        uint8_t in[64], want[32]; uint32_t m[16], h[8];
        for (int i = 0; i < 64; i++) in[i] = (uint8_t)(i * 37 + 11);
        plain_hash64(in, want);
        for (int i = 0; i < 16; i++) m[i] = (uint32_t)in[4 * i] | (uint32_t)in[4 * i + 1] << 8 | (uint32_t)in[4 * i + 2] << 16 | (uint32_t)in[4 * i + 3] << 24;
        hobbit::blake3_compress64(m, h);
        for (int i = 0; i < 32; i++)
            if (want[i] != (uint8_t)(h[i / 4] >> (8 * (i % 4)))) { fprintf(stderr, "blake3_compress64 differs from the plain compression at byte %d\n", i); return 1; }
    }
    const int Ks[3] = {1, 2, 32};
    for (int K : Ks) {
        std::vector<uint8_t> blk(64, 0), zdig(32), st(32, 0);        // heap blocks: the sanitizer sees every byte's bounds
        plain_hash64(blk.data(), zdig.data());
        for (int i = 0; i < K; i++) {
            memcpy(blk.data(), zdig.data(), 32); memcpy(blk.data() + 32, st.data(), 32);
            plain_hash64(blk.data(), st.data());
        }
        std::vector<uint32_t> z(8);
        hobbit::blake3_zero_group_leaf(K, z.data());
        printf("%d ", K);
        for (int i = 0; i < 32; i++) {
            const uint8_t b = (uint8_t)(z[i / 4] >> (8 * (i % 4)));
            if (b != st[i]) { fprintf(stderr, "\nZ_K differs from the plain loop: K = %d, byte %d\n", K, i); return 1; }
            printf("%02x", b);
        }
        printf("\n");
    }
    return 0;
}
