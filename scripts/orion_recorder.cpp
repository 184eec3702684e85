// scripts/orion_recorder.cpp -- TEST INFRASTRUCTURE ONLY: built by scripts/gen_orion_golden.py into a temporary directory and loaded (dlopen
// RTLD_GLOBAL) in FRONT of the real reference in a fresh child process that runs the reference's own test_PC(N, 2, K), behind oracle/_ref's
// libref_recorder_mimc.so (the mimc_hash call-through recorder, streaming to HOBBIT_REC_STREAM).
//
// Call-through interposers on the reference's Merkle entry points (src/merkle_tree.cpp).  The process dies on the first SHA3 call (inside the
// first _whir_prove of open_parity_matrix), so everything is written to files as it happens:
//   MT_commit_Blake   -- the FIRST call is commit_standard_orion's, over the flattened 2B x 2B tensor: its leaves (the tensor itself) go to
//                        HOBBIT_OR_TENSOR (u64 element count, then the elements) and the tree it built to HOBBIT_OR_COMMIT (u64 leaf count,
//                        then the flat levels).  Later calls (the column digests of shockwave_commit) only mark "inside".
//   create_tree_blake -- every tree built OUTSIDE MT_commit_Blake is appended to HOBBIT_OR_TREES (u64 leaf count, then the flat levels): the
//                        column trees of C, C_p and C_w, in that order.
//   open_tree_blake   -- the position c and the returned path of every call, appended to HOBBIT_OR_PATHS (u64 c[0], c[1], depth, then the
//                        path); the reference ends before it opens the commitment: what arrives are the column openings of
//                        shockwave_prove(C_p), and the generator asserts that.
// The few types it needs are declared here with the reference's layout: F = two 64-bit words, _hash = 32 bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
using std::vector;

namespace virgo { struct fieldElement { unsigned long long real, img; }; }
typedef virgo::fieldElement F;
struct _hash { uint8_t arr[32]; };

namespace merkle_tree {
namespace merkle_tree_prover {
void MT_commit_Blake(F *leafs, vector<vector<_hash>> &hashes, int N);
void create_tree_blake(int ele_num, vector<vector<_hash>> &hashes, const int element_size, bool alloc_required);
vector<_hash> open_tree_blake(vector<vector<_hash>> &MT_hashes, vector<size_t> c, int collumns);
}  // namespace merkle_tree_prover
}  // namespace merkle_tree

typedef void (*mt_commit_t)(F *, vector<vector<_hash>> &, int);
typedef void (*create_tree_t)(int, vector<vector<_hash>> &, const int, bool);
typedef vector<_hash> (*open_tree_t)(vector<vector<_hash>> &, vector<size_t>, int);
static mt_commit_t g_mt = nullptr;
static create_tree_t g_ct = nullptr;
static open_tree_t g_ot = nullptr;
static int g_inside_mt = 0;
static size_t g_mt_seen = 0;
static FILE *g_trees = nullptr, *g_paths = nullptr;

static void dump_levels(FILE *o, size_t n, const vector<vector<_hash>> &hashes) {
    const uint64_t n64 = n;
    fwrite(&n64, 8, 1, o);
    for (size_t l = 0, sz = n; l < hashes.size() && sz >= 1; l++, sz /= 2) fwrite(&hashes[l][0], 32, sz, o);
    fflush(o);
}

namespace merkle_tree {
namespace merkle_tree_prover {
void MT_commit_Blake(F *leafs, vector<vector<_hash>> &hashes, int N) {
    const bool first = g_mt_seen++ == 0;
    if (first) {
        if (const char *f = getenv("HOBBIT_OR_TENSOR")) {
            FILE *o = fopen(f, "wb");
            const uint64_t n = (uint64_t)N;
            fwrite(&n, 8, 1, o); fwrite(leafs, sizeof(F), n, o); fclose(o);
        }
    }
    g_inside_mt++;
    g_mt(leafs, hashes, N);
    g_inside_mt--;
    if (first) {
        if (const char *f = getenv("HOBBIT_OR_COMMIT")) { FILE *o = fopen(f, "wb"); dump_levels(o, (size_t)N / 4, hashes); fclose(o); }
    }
}
void create_tree_blake(int ele_num, vector<vector<_hash>> &hashes, const int element_size, bool alloc_required) {
    g_ct(ele_num, hashes, element_size, alloc_required);
    if (g_inside_mt || !g_trees) return;
    dump_levels(g_trees, (size_t)ele_num, hashes);
}
vector<_hash> open_tree_blake(vector<vector<_hash>> &MT_hashes, vector<size_t> c, int collumns) {
    vector<_hash> p = g_ot(MT_hashes, c, collumns);
    if (g_paths) {
        const uint64_t h[3] = {c[0], c[1], p.size()};
        fwrite(h, 8, 3, g_paths);
        if (!p.empty()) fwrite(&p[0], 32, p.size(), g_paths);
        fflush(g_paths);
    }
    return p;
}
}  // namespace merkle_tree_prover
}  // namespace merkle_tree

extern "C" void or_set_next(void *mt, void *ct, void *ot) {
    g_mt = (mt_commit_t)mt; g_ct = (create_tree_t)ct; g_ot = (open_tree_t)ot;
    const char *f = getenv("HOBBIT_OR_TREES"), *p = getenv("HOBBIT_OR_PATHS");
    if (f && !g_trees) g_trees = fopen(f, "wb");
    if (p && !g_paths) g_paths = fopen(p, "wb");
}
