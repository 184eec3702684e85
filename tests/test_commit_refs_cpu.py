"""tests/commit_refs.py against the oracle, wherever the oracle restates the same object: the quirk tree, the leaf chain and the tree of
commit_standard, the streaming leaves of elastic_commit, the column digests of shockwave_commit.  The conventional tree has no counterpart
in the oracle: every one of its paths is walked to the root by the library's host verifier.  No GPU."""
import ctypes
import numpy as np
import pytest
import commit_refs as cr
from oracle.pyoracle import splitmix_field


def rand_hashes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def test_tree_with_quirk_is_create_tree_blake(oracle):
    for n in (1, 2, 8, 4096):
        l0 = rand_hashes(n, 10 + n)
        got = cr.tree(l0, 1)
        assert got.shape == (2 * n - 1, 32)
        assert np.array_equal(got, oracle.create_tree_blake(l0)), n


def test_paths_is_open_tree_blake(oracle):
    n = 64
    lv = cr.tree(rand_hashes(n, 3), 1)
    pos = [0, 1, 31, 62, 63, 31]
    got = cr.paths(lv, n, pos)
    for q, p in enumerate(pos):
        assert np.array_equal(got[q], oracle.open_tree_blake(lv, n, p, 0, n)), p


@pytest.mark.parametrize("N,K,trs,lin", [(1 << 10, 4, 4, 0), (1 << 12, 2, 16, 0), (3 << 8, 3, 4, 0), (1 << 13, 1, 64, 1)])
def test_leaf_chain_is_commit_standard(oracle, N, K, trs, lin):
    if lin:
        oracle.rng_reset(); oracle.expander_init_store(trs)
    M = N // K
    lv, t = oracle.commit_standard(splitmix_field(N, 700 + K), K, trs, lin, want_tensor=True)
    T = np.ascontiguousarray(t.transpose(0, 2, 1, 3))                 # codeword-major, as the device keeps it
    leaves = cr.leaf_chain(T)
    assert np.array_equal(leaves, lv[:M])
    assert np.array_equal(cr.tree(leaves, 1), lv)
    # the chain in two parts, the inner digests chained by hand, and the slot order there and back
    if K > 1:
        assert np.array_equal(cr.leaf_chain(T[1:], cr.leaf_chain(T[:1])), leaves)
    dg = cr.inner_digests(T)
    st = np.zeros((M, 32), np.uint8)
    for i in range(K):
        st = oracle.blake3_64(np.concatenate([dg[i], st], axis=1))
    assert np.array_equal(st, leaves)
    assert np.array_equal(cr.chain_digests(dg), leaves)
    s0 = rand_hashes(M, K)
    assert np.array_equal(cr.chain_digests(dg, s0), cr.leaf_chain(T, s0))
    cols, half = 2 * M // trs, trs // 2
    so = cr.slot_order(leaves, cols, half)
    p = np.arange(M); g = (p % cols) * half + p // cols
    assert np.array_equal(so[g], leaves)


def test_elastic_leaves_is_elastic_commit(oracle):
    N, B = 1 << 15, 1 << 13
    chunk = oracle.read_stream_pc(B)                                  # the stream elastic_commit reads; every chunk alike
    t = oracle.compute_tensorcode(chunk, B >> 11, 0)
    want = oracle.elastic_commit(N, B, 1)
    leaves = cr.elastic_leaves([t] * (N // B), 1)
    assert np.array_equal(leaves, want[:4 * B])
    assert np.array_equal(cr.tree(leaves, 1), want)
    assert not np.array_equal(cr.elastic_leaves([t] * 4, 0), leaves)
    assert np.array_equal(cr.elastic_leaves([t] * 6, 1), leaves)     # a trailing half group is ignored


@pytest.mark.parametrize("k,w", [(4, 8), (16, 2), (64, 32)])
def test_col_digests_is_shockwave_commit(oracle, k, w):
    enc, lv = oracle.shockwave_commit(splitmix_field(k * w, 40 + k), k)
    assert np.array_equal(cr.col_digests(enc, k, 1), lv[:2 * w])
    if k > 4:
        assert not np.array_equal(cr.col_digests(enc, k, 0), lv[:2 * w])


def test_conventional_tree_verifies_on_the_host():
    from __graft_entry__ import load_package, build_hip
    build_hip()
    lib = load_package().load_library()
    lib.hobbit_verify_path_host.restype = ctypes.c_int
    V = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n, depth = 64, 6
    leaves = rand_hashes(n, 7)
    lv = cr.tree(leaves, 0)
    assert not np.array_equal(lv[n:], cr.tree(leaves, 1)[n:])
    root = np.ascontiguousarray(lv[-1])
    P = np.ascontiguousarray(cr.paths(lv, n, np.arange(n)))
    for pos in range(n):
        assert lib.hobbit_verify_path_host(V(leaves[pos]), pos, V(P[pos]), depth, V(root), 0) == 1, pos
        bad = leaves[pos].copy(); bad[pos % 32] ^= 1
        assert lib.hobbit_verify_path_host(V(bad), pos, V(P[pos]), depth, V(root), 0) == 0, pos
