// scripts/parity_recorder.cpp -- TEST INFRASTRUCTURE ONLY: built by scripts/gen_parity_golden.py into a temporary directory, against the
// reference's headers, and loaded (dlopen RTLD_GLOBAL) in FRONT of the real reference in a fresh child process, behind
// oracle/_ref's libref_recorder_mimc.so (the mimc_hash call-through recorder, streaming to HOBBIT_REC_STREAM).
//
// Ours: it declares the three reference functions of the parity-matrix family (src/sumcheck.cpp:2671-2885, 3201-3221) and the list builder
// they share (:2622-2669), calls them, and records what they produce:
//   create_tree_blake  -- call-through interposer; every tree built OUTSIDE MT_commit_Blake is appended to HOBBIT_PARITY_TREES at once
//                         (u64 leaf count, then the flat levels): the first is C_p's column tree, the second C_w's.  The file survives the
//                         end of open_parity_matrix, which dies on the unlinked SHA3 inside its first _whir_prove.
//   MT_commit_Blake    -- call-through; only marks "inside", since it builds a tree of its own through create_tree_blake.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "config_pc.hpp"
#include "sumcheck.h"
#include "utils.hpp"
#include "Virgo.h"
#include "merkle_tree.h"

void commit_parity_matrix(int n);                                                                                  // src/sumcheck.cpp:2671
void open_parity_matrix(vector<F> r1, vector<F> r2, int n, double &vt, double &ps);                                // :2708
proof prove_linear_code_batch(vector<vector<F>> &codewords, int n, double &vt, double &ps);                        // :3201
int generate_access_idx(vector<int> &access_idx1, vector<int> &access_idx2, vector<F> &weight, int Offset, int n, int dep, int &lvl);   // :2622
// expander_init_store and encode_monolithic are inline functions of the reference's headers: they are reached through oracle/ref_shim.cpp's entry points
// inside the reference library, so that this file instantiates no copy of its own (built with other flags)
extern "C" long long ref_expander_init_store(long long n);
extern "C" int ref_encode_monolithic(const uint64_t *src, uint64_t *dst, long long n);

typedef void (*mt_commit_t)(F *, vector<vector<_hash>> &, int);
typedef void (*create_tree_t)(int, vector<vector<_hash>> &, const int, bool);
static mt_commit_t g_mt = nullptr;
static create_tree_t g_ct = nullptr;
static int g_inside_mt = 0;
static FILE *g_trees = nullptr;

namespace merkle_tree {
namespace merkle_tree_prover {
void MT_commit_Blake(F *leafs, vector<vector<_hash>> &hashes, int N) {
    g_inside_mt++;
    g_mt(leafs, hashes, N);
    g_inside_mt--;
}
void create_tree_blake(int ele_num, vector<vector<_hash>> &hashes, const int element_size, bool alloc_required) {
    g_ct(ele_num, hashes, element_size, alloc_required);
    if (g_inside_mt || !g_trees) return;
    const uint64_t n = (uint64_t)ele_num;
    fwrite(&n, 8, 1, g_trees);
    for (size_t l = 0, sz = (size_t)ele_num; l < hashes.size() && sz >= 1; l++, sz /= 2) fwrite(&hashes[l][0], 32, sz, g_trees);
    fflush(g_trees);
}
}  // namespace merkle_tree_prover
}  // namespace merkle_tree

extern "C" {
void pr_set_next(void *mt, void *ct) {
    g_mt = (mt_commit_t)mt; g_ct = (create_tree_t)ct;
    const char *f = getenv("HOBBIT_PARITY_TREES");
    if (f && !g_trees) g_trees = fopen(f, "wb");
}
// the lists of generate_access_idx for the graphs expander_init_store(n) left: returns m; idx1 / idx2 (m ints), weight (m F) when non-null
size_t pr_lists(int n, int *idx1, int *idx2, uint64_t *weight) {
    vector<int> a1, a2; vector<F> w; int lvl = 0;
    generate_access_idx(a1, a2, w, 0, n, 0, lvl);
    if (idx1) memcpy(idx1, a1.data(), 4 * a1.size());
    if (idx2) memcpy(idx2, a2.data(), 4 * a2.size());
    if (weight) memcpy(weight, w.data(), 16 * w.size());
    return a1.size();
}
long long pr_graphs(int n) { return ref_expander_init_store(n); }
void pr_commit(int n) { commit_parity_matrix(n); }
// r1, r2 = generate_randomness(log2 2n) each, as a caller of open_parity_matrix draws them; does not return (SHA3 is not linked)
void pr_open(int n, uint64_t *r12_out) {
    const int l = (int)log2(2 * n);
    vector<F> r1 = generate_randomness(l), r2 = generate_randomness(l);
    memcpy(r12_out, r1.data(), 16 * (size_t)l); memcpy(r12_out + 2 * l, r2.data(), 16 * (size_t)l);
    FILE *f = fopen(getenv("HOBBIT_PARITY_R12"), "wb"); fwrite(r12_out, 16, 2 * (size_t)l, f); fclose(f);
    double vt = 0, ps = 0;
    open_parity_matrix(r1, r2, n, vt, ps);
}
// `count` codewords: encode_monolithic of generate_randomness(n) each (2n F: the codeword, then zeros), then the batch proof.
// out: cw (count x 2n F), q (rounds x 3 F), r (rounds F), vr (2 F), fin (1 F), r1 (log2 2n F), r2 (log2 count F); returns the rounds
int pr_batch(int n, int count, uint64_t *cw, uint64_t *q, uint64_t *r, uint64_t *vr, uint64_t *fin, uint64_t *r1, uint64_t *r2) {
    vector<vector<F>> cws(count);
    for (int i = 0; i < count; i++) {
        vector<F> msg = generate_randomness(n);
        cws[i].assign(2 * (size_t)n, F(0));
        ref_encode_monolithic((const uint64_t *)msg.data(), (uint64_t *)cws[i].data(), n);
        memcpy(cw + (size_t)i * 4 * n, cws[i].data(), 32 * (size_t)n);
    }
    double vt = 0, ps = 0;
    proof P = prove_linear_code_batch(cws, n, vt, ps);
    for (size_t i = 0; i < P.q_poly.size(); i++) {
        memcpy(q + 6 * i, &P.q_poly[i].a, 16); memcpy(q + 6 * i + 2, &P.q_poly[i].b, 16); memcpy(q + 6 * i + 4, &P.q_poly[i].c, 16);
        memcpy(r + 2 * i, &P.randomness[0][i], 16);
    }
    memcpy(vr, &P.vr[0], 16); memcpy(vr + 2, &P.vr[1], 16); memcpy(fin, &P.final_rand, 16);
    memcpy(r1, P.randomness[1].data(), 16 * P.randomness[1].size()); memcpy(r2, P.randomness[2].data(), 16 * P.randomness[2].size());
    return (int)P.q_poly.size();
}
}
