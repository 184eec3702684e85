// scripts/brakedown_recorder.cpp -- TEST INFRASTRUCTURE ONLY: built by scripts/gen_brakedown_golden.py into a temporary directory and loaded
// (dlopen RTLD_GLOBAL) in FRONT of the real reference (oracle/_ref/libhobbit_ref.so), in a child process that runs test_PC(N, 3, K).
// scripts/gen_brakedown_stream_golden.py uses it the same way around test_Elastic_PC(N, 3): commit_brakedown_stream and
// open_brakedown_stream (src/Elastic_PC.cpp:112-172, 561-623) go through the same four entry points in the same order.
//
// Call-through interposers on the reference's Merkle entry points (src/merkle_tree.cpp) record what commit_standard_brakedown and
// open_brakedown_standard (src/Our_PC.cpp:197-236, 432-520) produce:
//   create_tree_blake      -- outside MT_commit_Blake and before the open: the commitment's levels (the tree over the 2B column digests)
//   open_tree_blake        -- the queried column c[1] = I[q] and the returned path; the first call marks the start of the open
//   MT_commit_Blake        -- once the open has begun: the reply rows the verifier re-commits
//   verify_claim_opt_blake -- a stand-in: the real one ends in SHA3 (my_hhash, from a prebuilt library that is not linked), so it keeps
//                             only the proof-size accounting of src/merkle_tree.cpp:326-361 (32 B per sibling not yet visited)
// The few types it needs are declared here with the reference's layout: F = two 64-bit words, _hash = 32 bytes.
#include <cstdint>
#include <cstring>
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
namespace merkle_tree_verifier {
bool verify_claim_opt_blake(vector<vector<_hash>> &MT, const _hash *path, int pos_element_arr, int N, bool *visited, double &ps);
}  // namespace merkle_tree_verifier
}  // namespace merkle_tree

typedef void (*mt_commit_t)(F *, vector<vector<_hash>> &, int);
typedef void (*create_tree_t)(int, vector<vector<_hash>> &, const int, bool);
typedef vector<_hash> (*open_tree_t)(vector<vector<_hash>> &, vector<size_t>, int);
static mt_commit_t g_mt = nullptr;
static create_tree_t g_ct = nullptr;
static open_tree_t g_ot = nullptr;

static int g_inside_mt = 0;
static bool g_open = false;
static vector<uint8_t> g_levels;           // flat: level 0 .. root
static size_t g_leaves = 0;
static vector<uint64_t> g_I;
static vector<uint8_t> g_paths;
static size_t g_depth = 0;
static vector<F> g_replies;
static size_t g_reply_len = 0;
static double g_ps = 0.0;

namespace merkle_tree {
namespace merkle_tree_prover {
void MT_commit_Blake(F *leafs, vector<vector<_hash>> &hashes, int N) {
    if (g_open) { g_replies.insert(g_replies.end(), leafs, leafs + N); g_reply_len = (size_t)N; }
    g_inside_mt++;
    g_mt(leafs, hashes, N);
    g_inside_mt--;
}
void create_tree_blake(int ele_num, vector<vector<_hash>> &hashes, const int element_size, bool alloc_required) {
    g_ct(ele_num, hashes, element_size, alloc_required);
    if (g_inside_mt || g_open) return;
    g_levels.clear(); g_leaves = (size_t)ele_num;
    for (size_t l = 0, sz = (size_t)ele_num; l < hashes.size() && sz >= 1; l++, sz /= 2)
        for (size_t i = 0; i < sz; i++) g_levels.insert(g_levels.end(), hashes[l][i].arr, hashes[l][i].arr + 32);
}
vector<_hash> open_tree_blake(vector<vector<_hash>> &MT_hashes, vector<size_t> c, int collumns) {
    g_open = true;
    vector<_hash> p = g_ot(MT_hashes, c, collumns);
    g_I.push_back(c[1]); g_depth = p.size();
    for (auto &h : p) g_paths.insert(g_paths.end(), h.arr, h.arr + 32);
    return p;
}
}  // namespace merkle_tree_prover
namespace merkle_tree_verifier {
bool verify_claim_opt_blake(vector<vector<_hash>> &MT, const _hash *path, int pos_element_arr, int N, bool *visited, double &ps) {
    (void)path;
    int pos_element = N + pos_element_arr;
    for (size_t i = 0; i + 1 < MT.size(); i++) {
        if (visited[pos_element ^ 1]) return true;
        visited[pos_element ^ 1] = true;
        pos_element /= 2;
        visited[pos_element] = true;
        ps += 32.0 / 1024.0; g_ps += 32.0 / 1024.0;
    }
    return true;
}
}  // namespace merkle_tree_verifier
}  // namespace merkle_tree

extern "C" {
void rec_set_next(void *mt, void *ct, void *ot) { g_mt = (mt_commit_t)mt; g_ct = (create_tree_t)ct; g_ot = (open_tree_t)ot; }
size_t rec_leaves(void) { return g_leaves; }
void rec_levels(uint8_t *out) { memcpy(out, g_levels.data(), g_levels.size()); }
size_t rec_queries(void) { return g_I.size(); }
size_t rec_depth(void) { return g_depth; }
void rec_I(uint64_t *out) { memcpy(out, g_I.data(), 8 * g_I.size()); }
void rec_paths(uint8_t *out) { memcpy(out, g_paths.data(), g_paths.size()); }
size_t rec_reply_count(void) { return g_reply_len ? g_replies.size() / g_reply_len : 0; }
size_t rec_reply_len(void) { return g_reply_len; }
void rec_replies(F *out) { memcpy(out, g_replies.data(), sizeof(F) * g_replies.size()); }
double rec_ps_paths(void) { return g_ps; }
}
