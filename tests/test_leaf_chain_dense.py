"""The commit's leaf chain over the dense index of the non-zero leaf groups (k_leaf_chain): the groups j >= zero_from = (code.len + 3) / 4 of
an RS x expander tensor are zero in every chunk, the kernel leaves them out of its index space (idx in [0, cols * zero_from), c = idx /
zero_from, j = idx % zero_from) and stores the host-computed constant Z_K (tests/test_leaf_chain_zero_groups_cpu.py) into their leaves, one
contiguous tail of the leaf array with the Merkle levels right behind it.

Everything goes through hb.commit_standard, and ALL Merkle levels are compared byte for byte with oracle.commit_standard.  Each shape is the
smallest that reaches one way the indexing can go wrong (SHAPES).  Every case commits twice: the first commitment's levels buffer is filled with
a sentinel through its device pointer and parked, the second commit of the same shape re-uses it, so every level must have been written again and
the slot behind the last level (the 2M-th of the 2M the buffer has) must come back untouched."""
import ctypes

import numpy as np
import pytest

import commit_refs as cr
from adversarial import graphs_from
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
SENT = 0xA5

# (N, K, trs, lin): what it reaches.  Codeword lengths: trs 16 -> 27, 256 -> 440, 1024 -> 1761, so zero_from is 7 of 8, 110 of 128, 441 of 512.
SHAPES = [
    (256, 1, 16, 1),          # zero_from 7 of 8; the dense range (224) is under one workgroup; waves straddle nine columns; the fill is 32 leaves
    (3 << 12, 3, 16, 1),      # same geometry, 14 full workgroups, K = 3 (Z_K depends on K)
    (1 << 15, 1, 1024, 1),    # zero_from 441 (odd); dense range 28 224 = 110 workgroups + 64 leaves: ragged last workgroup; K = 1
    (1 << 17, 2, 256, 1),     # zero_from 110; 220 workgroups; fill of 18 * 512 leaves
    (1 << 22, 2, 1024, 1),    # dense range of 7056 workgroups, more than any grid the launcher may pick: a workgroup walks several passes
    (1 << 12, 4, 16, 0),      # RS x RS, no zero group: the dense range is the whole range, no fill, no Z_K
    (64, 2, 8, 1),            # trs <= 13: the code is finalised inside the commit; whatever code.len is there, the levels must match
]
ORACLE_TOO_SLOW = {(1 << 22, 2, 1024, 1)}      # 4.5 s of single-thread oracle: compared with the host chain and tree over the device's own tensor


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def set_graphs(hb, oracle, trs, lin):
    if not lin:
        return
    oracle.rng_reset(); oracle.expander_init_store(trs)
    if trs > 13:
        hb.upload_graphs(trs, graphs_from(oracle, trs))
    else:
        hb._chk(hb.lib.hobbit_graph_reset(hb.ctx))                   # nothing finalised: the commit does it


def commit_into_dirty_levels(hb, poly, K, trs, lin):
    """commit, fill the whole levels buffer (2M slots) with the sentinel, park it, commit again into it: (the commitment, its levels, whether
    the buffer was re-used, whether the 2M-th slot still holds the sentinel)"""
    c0 = hb.commit_standard(poly, K, trs, lin)
    M = c0.M
    ptr0 = hb.lib.hobbit_commitment_levels_dev(c0.h)
    hb._chk(hb.lib.hobbit_memset(hb.ctx, ptr0, SENT, 64 * M)); hb.sync()
    c0.free()
    c = hb.commit_standard(poly, K, trs, lin)
    ptr = hb.lib.hobbit_commitment_levels_dev(c.h)
    last = hb.to_host(ptr, (32,), np.uint8, 32 * (2 * M - 1))
    return c, c.levels(), ptr == ptr0, bool((last == SENT).all())


@pytest.mark.parametrize("N,K,trs,lin", SHAPES, ids=lambda v: str(v))
def test_commit_levels_every_dense_geometry(hb, oracle, N, K, trs, lin):
    set_graphs(hb, oracle, trs, lin)
    poly = splitmix_field(N, 2600 + K + trs)
    c, levels, reused, intact = commit_into_dirty_levels(hb, poly, K, trs, lin)
    try:
        assert reused, "the second commit did not re-use the parked buffers"
        assert intact, "the slot behind the last level was written"
        if (N, K, trs, lin) in ORACLE_TOO_SLOW:
            T = np.ascontiguousarray(c.tensor().transpose(0, 2, 1, 3))        # (K, 2 trs, cols, 2) -> codeword-major
            want = cr.tree(cr.leaf_chain(T), 1)
            assert T[:, :, 1760].any() and not T[:, :, 1761:].any()           # the codeword length at trs = 1024 is 1761: the rows behind it read as zeros
        else:
            want, _ = oracle.commit_standard(poly, K, trs, lin)
        assert levels.shape == want.shape
        bad = np.flatnonzero((levels != want).any(axis=1))
        assert bad.size == 0, "first differing node %d of %d (M = %d)" % (bad[0], len(want), c.M)
    finally:
        c.free()


def test_two_commits_with_different_k(hb, oracle):
    """K = 3, then K = 1 at the same M and trs, then K = 3 again: a Z_K kept from another K, or a fill left from an earlier commit, would show.
    (The parked buffers are re-used only by a commit of the same byte sizes, which fixes K; the commit with the other K releases them and
    allocates its own, as a caller changing K meets it.)"""
    trs, M = 16, 1 << 12
    set_graphs(hb, oracle, trs, 1)
    seen = {}
    for K in (3, 1, 3):
        poly = splitmix_field(K * M, 2700 + K)
        c, levels, reused, intact = commit_into_dirty_levels(hb, poly, K, trs, 1)
        try:
            assert reused and intact
            want, _ = oracle.commit_standard(poly, K, trs, 1)
            assert np.array_equal(levels, want), K
            tail = levels[7 * c.cols:M]                                       # the leaves of group 7 of 8
            assert (tail == tail[0]).all()
            seen.setdefault(K, tail[0].copy())
            assert np.array_equal(seen[K], tail[0])
        finally:
            c.free()
    assert not np.array_equal(seen[1], seen[3])
