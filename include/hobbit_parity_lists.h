/* hobbit_parity_lists.h -- third header of the parity matrix' commitment in libhobbit_hip.so: the access lists of generate_access_idx
 * (src/sumcheck.cpp:2622-2669) built on the device.  hobbit_parity_commit (hobbit_parity.h) restates the reference's host loop and stays the
 * independent check of this path; the objects of both are the same type and go through the same accessors and hobbit_parity_open.
 * Conventions are those of hobbit_hip.h (device pointers d_*, host pointers h_*, stream semantics, error codes).
 */
#ifndef HOBBIT_PARITY_LISTS_H
#define HOBBIT_PARITY_LISTS_H
#include "hobbit_parity.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hobbit_parity_commit with the lists built by kernels: same range of n (a power of two, 16 <= n <= 2^21), same refusals with the same codes,
 * and every byte the object owns -- idx1, idx2, cnt1, cnt2, weight, acc1, acc2, the 8P public witness, the encoded rows, the tree -- equal to
 * what hobbit_parity_commit produces for the same graphs.  The lists are a function of the finalized code alone: its forward form (every
 * level's neighbours and weights in list order, and a table of the list's segments) is uploaded by the first such commit after
 * hobbit_graph_finalize and kept with the code; the index ranges are checked from that table before any launch (HOBBIT_EINVAL).
 * Asynchronous on the context's stream; draws nothing from libc; the object owns no host memory.  hobbit_parity_dims' list_seconds is the host
 * wall time of this call up to the point where the list kernels are queued (shape, first-use upload, scratch, launches). */
int hobbit_parity_commit_device(hobbit_ctx *ctx, long long n, hobbit_parity_commitment **out);

/* m (the number of list entries) and P (the next power of two) of the code finalized for n, from the levels' (L, degree, R).  Host only: no
 * allocation, launch or draw.  The refusals of the commit that need no list entry: n out of range or a list outside the public witness' 8P
 * layout (HOBBIT_EINVAL), graphs not finalized for n (HOBBIT_ESTATE).  Either pointer may be NULL. */
int hobbit_parity_shape(hobbit_ctx *ctx, long long n, size_t *m, size_t *P);

#ifdef __cplusplus
}
#endif
#endif
