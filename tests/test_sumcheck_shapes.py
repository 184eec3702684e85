"""The sparse 2-product sumcheck on its own (hobbit_sumcheck2_sparse: the opening's P3) and every size class of the dense sumchecks.

k_sc2_sparse_round scans, folds and regroups a sorted (index, value) list in one workgroup; through the opening it only ever sees lists
of about 5900 uniform positions.  Here it gets the lists of tests/adversarial.py (SPARSE_PURPOSE), at the smallest sparse size and at an
odd and an even number of two-round trips.  The dense 2- and 3-product sumchecks and the gate sumcheck run at every size from the
host-only ones to 2^21, and the whole opening at query counts from 1 to 200000.  Integer work throughout: every comparison is bit for
bit against the oracle, which the committed fixtures pin to the reference."""
import ctypes
import numpy as np
import pytest
from adversarial import (families, sparse_lists, short_sparse_lists, open_like_list, pm1_with_zeros, scatter_dense, with_kernels,
                         gate_sumcheck_inputs, graphs_from)
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
PREV_R = np.array([121, 0], np.uint64)          # P3's transcript seed (src/PC_utils.cpp:339)
SC_KEYS = ("poly", "r", "vr", "fin")
SPARSE_KERNELS = {"k_sc2_sparse_round", "k_sc2_fold4", "k_scatter_counted"}


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def same(got, want, what):
    for k in SC_KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


def sparse_vs_oracle(hb, oracle, v1, idx, val, what, profiled=False):
    """the sparse form on (idx, val) against the oracle on the scattered table; returns the kernel names when profiled"""
    v2 = scatter_dense(v1.shape[0], idx, val)
    want = oracle.sumcheck2(v1, v2, PREV_R)
    run = lambda: hb.generate_2product_sumcheck_proof_sparse(v1, idx, val, PREV_R)
    got, names = with_kernels(hb, run) if profiled else (run(), None)
    same(got, want, what)
    return names, v2, want


# ---- a. the list structures, at the sizes that take the sparse form -----------------------------------------------------------------
@pytest.mark.parametrize("logn", [18, 19, 20])
def test_sumcheck2_sparse_list_structures(hb, oracle, logn):
    """2^18 is the smallest table that takes the sparse form (16 SC_DOUBLE_MIN); 2^19 and 2^20 make an odd and an even number of
    two-round trips, which decides where the bridge finds its buffers."""
    n = 1 << logn
    v1 = splitmix_field(n, 500 + logn)
    lists = sparse_lists(n, seed=logn)
    fam = families(n, seed=logn)
    assert len(lists["full_quads"]) == 1200 and len(lists["odd_run"]) == (1 << 16) + 3 and len(lists["max_spread"]) == n // 4
    for name, idx in lists.items():
        what = "n=2^%d %s (m=%d)" % (logn, name, len(idx))
        val = open_like_list(n, seed=logn)[1] if name == "open_like" else splitmix_field(len(idx), 600 + logn)
        names, v2, want = sparse_vs_oracle(hb, oracle, v1, idx, val, what, profiled=(name == "open_like"))
        if name == "open_like":
            # the path under test is the one that ran: a changed threshold fails here instead of testing the dense kernels
            assert SPARSE_KERNELS <= names and "k_sc2_double" not in names, "%s: kernels %s" % (what, sorted(names))
            same(hb.generate_2product_sumcheck_proof(v1, v2, PREV_R), want, what + " dense on the device")
        if name in ("full_quads", "odd_run", "open_like"):
            sparse_vs_oracle(hb, oracle, v1, idx, pm1_with_zeros(len(idx)), what + " values p-1 and zeros")
        if name in ("full_quads", "open_like"):
            for f in ("all_pm1", "zeros", "bits"):
                sparse_vs_oracle(hb, oracle, fam[f], idx, val, what + " v1=" + f)


# ---- b. tables short enough to be scattered at once ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 16, 1024, 1 << 11, 1 << 14, 1 << 17])
def test_sumcheck2_sparse_short_tables(hb, oracle, n):
    """the host tail's scatter (n <= 1024), round by round, one two-round trip (2^14), and the largest size that still scatters at once"""
    v1 = splitmix_field(n, 700)
    for name, idx in short_sparse_lists(n, seed=n.bit_length()).items():
        what = "n=%d %s (m=%d)" % (n, name, len(idx))
        names, _, _ = sparse_vs_oracle(hb, oracle, v1, idx, splitmix_field(len(idx), 701), what, profiled=True)
        assert "k_sc2_sparse_round" not in names, "%s: kernels %s" % (what, sorted(names))


# ---- c. what the launcher refuses ----------------------------------------------------------------------------------------------------
def test_sumcheck2_sparse_bad_arguments(hb, oracle):
    """refused before anything is launched: an empty list, one longer than 2^20 or than the table, a table that is no power of two; and
    an opening asked for 2^20 queries.  (Unsorted lists and indices past the table are the caller's contract: not passed here.)"""
    from __graft_entry__ import load_package
    E = load_package().HobbitError
    lib, ctx = hb.lib, hb.ctx
    d = hb.to_device(splitmix_field(1 << 12, 1))
    out = [np.zeros((64, 3, 2), np.uint64), np.zeros((64, 2), np.uint64), np.zeros((2, 2), np.uint64), np.zeros(2, np.uint64)]
    o = [a.ctypes.data_as(ctypes.c_void_p) for a in out]
    pr = PREV_R.ctypes.data_as(ctypes.c_void_p)
    for m, n, word in ((0, 1 << 12, b"non-zeros"), ((1 << 20) + 1, 1 << 21, b"non-zeros"), (17, 16, b"non-zeros"), (4097, 4096, b"non-zeros"),
                       (10, 1000, b"power of two")):
        assert lib.hobbit_sumcheck2_sparse(ctx, d.ptr, d.ptr, d.ptr, m, n, pr, *o) < 0, (m, n)
        assert word in lib.hobbit_last_error(ctx), (m, n, lib.hobbit_last_error(ctx))
    assert all(not a.any() for a in out)
    with pytest.raises(E, match="bad arguments"):
        hb.open_from_aggregate(splitmix_field(1 << 13, 2), 4, 4, queries=1 << 20)
    # the context is still usable afterwards
    assert np.array_equal(hb.precompute_beta(splitmix_field(6, 2)), oracle.precompute_beta(splitmix_field(6, 2)))


# ---- d. every size class of the dense sumchecks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", list(range(1, 22)))
def test_sumchecks_every_size(hb, oracle, logn):
    """host only up to 2^10, round by round up to 2^13, two rounds per trip from 2^14 with the bridge's buffers at either parity of
    the trip count; uniform data and the small-integer mix of tests/adversarial.py.  The gate sumcheck from 2^4 to 2^20."""
    n = 1 << logn
    pr = splitmix_field(1, 900 + logn)[0]
    mix = [families(n, seed=s)["mix"] for s in (1, 2, 3)]
    inputs = {"uniform": [splitmix_field(n, 910 + 3 * logn + j) for j in range(3)],
              "mix": [mix[0], np.ascontiguousarray(mix[1][::-1]), np.roll(mix[2], n // 3, axis=0)]}       # (the blocks of the three tables do not line up)
    for name, (a, b, c) in inputs.items():
        what = "n=2^%d %s" % (logn, name)
        same(hb.generate_2product_sumcheck_proof(a, b, pr), oracle.sumcheck2(a, b, pr), what + " sumcheck2")
        same(hb.generate_3product_sumcheck_proof(a, b, c, pr), oracle.sumcheck3(a, b, c, pr), what + " sumcheck3")
    if 4 <= logn <= 20:
        tabs, a, rand0 = gate_sumcheck_inputs(n)
        claim = oracle.gate_claim(tabs, a)
        want = oracle.gate_sumcheck(tabs, a, rand0, claim)
        got = hb.gate_sumcheck(tabs, a, rand0, claim)
        assert want["check"].tolist() == [1] and got["check"].tolist() == [1], "n=2^%d gate: the reference's round check" % logn
        for k in ("poly", "r", "fin", "rand", "sum"):
            assert np.array_equal(got[k], want[k]), "n=2^%d gate: %s differs" % (logn, k)
        bad = claim.copy(); bad[0] ^= np.uint64(1)
        assert hb.gate_sumcheck(tabs, a, rand0, bad)["check"].tolist() == [0], "n=2^%d gate: a flipped claim passed" % logn


# ---- e. the whole opening at list lengths it has not seen ----------------------------------------------------------------------------
SP_KEYS = ("I", "q1", "r1", "vr1", "fin1", "q2", "r2", "vr2", "fin2", "iters", "wq", "wa", "wroots", "wscal", "wchecks", "whir_root",
           "reply", "paths", "qn", "qidx", "qreply", "qpaths", "final_pb")
_COMMITS = {}


def open_case(oracle, N, K):
    """test_open_standard_vs_oracle's case: the libc sequence poly, graphs, x on the oracle (which leaves ITS graphs at this trs); the
    oracle's commitment of the polynomial is computed once per shape"""
    trs = N // (K << 11)
    oracle.rng_reset(); poly = oracle.generate_randomness(N); oracle.expander_init_store(trs)
    x = oracle.generate_randomness(N.bit_length() - 1)
    if (N, K) not in _COMMITS:
        _COMMITS[(N, K)] = oracle.commit_standard(poly, K, trs, 1, want_tensor=True)
    return (trs, poly, x) + _COMMITS[(N, K)]


@pytest.mark.parametrize("queries", [1, 2, 1000, 1024, 20000, 200000])
@pytest.mark.parametrize("N,K", [(1 << 18, 4), (1 << 20, 4)])
def test_open_standard_query_counts(hb, oracle, N, K, queries):
    """the two smallest shapes whose P3 table (big = 2 trs * 4096 = 2^18, 2^20) takes the sparse form, with buff2 from one entry to
    139822 (of 2^18) and 182042 (of 2^20) distinct positions"""
    libc = ctypes.CDLL(None)
    trs, poly, x, lv, T = open_case(oracle, N, K)
    assert 2 * trs * 4096 == N
    libc.srandom(777); want = oracle.open_standard(poly, K, trs, x, queries, tensor=T)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    c = hb.commit_standard(poly, K, trs, 1)
    paths = queries <= 20000                                    # (200000 of them would be 100 MB)
    libc.srandom(777); got = hb.open_standard(poly, c, x, queries, want_paths=paths)
    assert want["checks"].tolist() == [1, 1, 1] and got["checks"].tolist() == [1, 1, 1]
    for k in ("I", "scalars", "poly", "r", "vr", "fin", "roots"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["reply"], want["reply"])
    if paths:
        M = N // K
        for q in range(0, queries, 97):
            assert np.array_equal(got["paths"][q], oracle.open_tree_blake(lv, M, int(got["I"][q, 0]), int(got["I"][q, 1]), 4096)), q
    for sp in ("sp_c", "sp_f"):
        has_whir = int(want[sp]["iters"][0]) > 0
        assert want[sp]["wchecks"].tolist() == ([1, 1] if has_whir else [0, 0]), sp
        for k in SP_KEYS:
            assert np.array_equal(got[sp][k], want[sp][k]), (sp, k)
    c.free()
