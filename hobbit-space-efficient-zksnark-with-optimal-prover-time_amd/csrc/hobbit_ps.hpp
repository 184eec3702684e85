// hobbit_ps.hpp -- the reference's proof-size accounting (KB), piece by piece as it adds it, shared by the baselines that restate it
// (hobbit_brakingbase.hip, hobbit_orion.hip).  Host only.
#pragma once
#include <vector>
#include "../../include/hobbit_hip.h"

namespace hobbit_ps {

inline int ilog2x(size_t n) { int l = 0; while (((size_t)1 << l) < n) l++; return ((size_t)1 << l) == n ? l : -1; }

// Every term is a multiple of 1/64, so the sums are exact.
constexpr double FKB = sizeof(hobbit_F) / 1024.0;
// verify_claim_opt_blake (src/merkle_tree.cpp:326-361): 32 B per sibling not yet seen
template <class T>
inline void path_ps(size_t n_leaves, int depth, const T *pos, size_t npos, double &ps) {
    std::vector<bool> visited(2 * n_leaves + 2, false);
    for (size_t q = 0; q < npos; q++) {
        size_t pe = n_leaves + (size_t)pos[q];
        for (int i = 0; i < depth; i++) {
            if (visited[pe ^ 1]) break;
            visited[pe ^ 1] = true; pe /= 2; visited[pe] = true;
            ps += 32.0 / 1024.0;
        }
    }
}
inline void sumcheck2_ps(int rounds, double &ps) { for (int i = 0; i < rounds; i++) ps += 3 * FKB; ps += 2 * FKB; }       // src/sumcheck.cpp:2431, 2449
inline void sumcheck3_ps(int rounds, double &ps) { ps += ((size_t)rounds * 5 + 3) * FKB; }                                // src/sumcheck.cpp:2031, 2048
// one shockwave_prove (src/Virgo.cpp:435-517) with its _whir_prove (:519-686) on w = N / k coefficients when w > 256
inline void shockwave_ps(const hobbit_shockwave_out *o, size_t N, int k, double &ps) {
    const size_t w = N / k, W = 2 * w; const int lgW = ilog2x(W);
    sumcheck2_ps(lgW, ps); sumcheck2_ps(lgW, ps);
    if (w > 256) {
        const int iters = *o->iters; size_t q = 0;
        for (int it = 1; it <= iters; it++) {
            for (int i = 0; i < 4; i++) ps += 3 * FKB;
            const size_t size = it == 1 ? 2 * w : (2 * w) >> (it - 1);
            if (it == iters) ps += (w >> (4 * iters)) * 2 * FKB;
            const int n = o->wqn[it - 1];
            ps += 16.0 * n * FKB;
            path_ps(size / 4, ilog2x(size / 4), o->wqidx + q, (size_t)n, ps);
            q += (size_t)n;
        }
    } else ps += 2 * w * FKB;
    ps += 240.0 * k * FKB;
    path_ps(W, lgW, o->I, 240, ps);
}
inline bool sp_has_queries(const hobbit_shockwave_out *o) { return o && o->I && o->wqidx && o->wqn && o->iters; }


}  // namespace hobbit_ps
