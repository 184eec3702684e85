"""Openings made on the device verify: tests/open_verifier.py run on hobbit_open_standard (RS x expander) and hobbit_shockwave_prove.

What the bit-for-bit tests against the oracle cannot say at the shapes the oracle cannot reach -- (2^26, 32), (2^24, 2), the benchmark's (2^28, 32) --
this file says without it: the sumchecks chain into each other, their final values are what a verifier computes from public data, and the query
replies are what the sumchecks were run on.  The two ends of an opening are evaluations of the device's own aggregate (hobbit_aggregate on the
device polynomial, read back; 64 seeded entries of it are recomputed in Python integers from polynomial elements read back from the device):
  * M = N / K <= 2^21: by the oracle's compute_tensorcode and evaluate_vector on the CPU ("oracle_ends");
  * M = 2^23: by hobbit_tensorcode and hobbit_eval_vector ("device_ends"), kernels pinned elsewhere and none of them the sumcheck's.
"""
import ctypes
import time

import numpy as np
import pytest

import brakingbase_model as bm
import open_verifier as ov
from open_verifier import Rejected, fi
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
libc = ctypes.CDLL(None)
c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t
COLS = 4096


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


def _p(a):
    return a.ctypes.data_as(c_vp)


def dev_eval(hb, ptr, n, r):
    r = np.ascontiguousarray(r, np.uint64); o = np.zeros(2, np.uint64)
    assert 1 << len(r) == n
    hb._chk(hb.lib.hobbit_eval_vector(hb.ctx, c_vp(ptr), c_sz(n), _p(r), _p(o)))
    return o


def device_aggregate(hb, d, N, K, x):
    """hobbit_aggregate of the device polynomial with eq(x[:log2 K]) from Python integers: (device buffer, host copy); 64 seeded entries of
    it are recomputed in Python integers from polynomial elements read back one by one"""
    M = N // K
    beta = [ov.eq_at(x[:K.bit_length() - 1], i) for i in range(K)]
    hbeta = np.array(beta, np.uint64)
    d_aggr = hb.alloc(16 * M)
    hb._chk(hb.lib.hobbit_aggregate(hb.ctx, c_vp(d.ptr), c_sz(N), _p(hbeta), K, c_vp(d_aggr.ptr)))
    hb.sync()
    aggr = hb.to_host(d_aggr, (M, 2), np.uint64)
    picks = [0, M - 1] + np.random.default_rng(N + K).integers(0, M, 62).tolist()
    for j in picks:
        want = ov.ZERO
        for i in range(K):
            want = ov.fadd(want, ov.fmul(beta[i], fi(hb.to_host(d, (2,), np.uint64, offset=16 * (i * M + j)))))
        assert fi(aggr[j]) == want, "aggregate entry %d" % j
    return d_aggr, aggr


def oracle_evaluators(oracle, aggr, trs):
    """C~ and aggr~ on the CPU: C the parity half of the oracle's tensor code of the device's aggregate, row-major"""
    C = np.ascontiguousarray(oracle.compute_tensorcode(aggr, trs, 1).reshape(2 * trs, COLS, 2)[trs:].reshape(-1, 2))
    return (lambda p: oracle.evaluate_vector(C, p)), (lambda p: oracle.evaluate_vector(aggr, p))


def device_evaluators(hb, d_aggr, M, trs):
    """C~ and aggr~ by hobbit_tensorcode and hobbit_eval_vector.  The device's tensor is codeword-major, element (row, col) at col * 2 trs + row, so
    a point (col | row) over C's row-major index is (row | 1 | col) over the device's: the 1 picks the parity half"""
    d_T = hb.alloc(16 * 4 * M)
    hb._chk(hb.lib.hobbit_tensorcode(hb.ctx, c_vp(d_aggr.ptr), c_sz(M), trs, 1, c_vp(d_T.ptr)))
    hb.sync()
    logc = COLS.bit_length() - 1

    def evalC(p):
        return dev_eval(hb, d_T.ptr, 4 * M, np.concatenate([p[logc:], np.array([[1, 0]], np.uint64), p[:logc]]))
    return evalC, (lambda p: dev_eval(hb, d_aggr.ptr, M, p)), d_T


def commit_and_open(hb, oracle, logN, K, queries, where, seed, change=None):
    """graphs, commitment and opening of fill_splitmix(N) on the device; change: one bit of one coefficient flipped between commit and open.
    Returns the opening, the point, trs and (evalC, evalA) over the aggregate of the polynomial that was opened"""
    N = 1 << logN; trs = N // (K << 11); M = N // K
    if where == "oracle_ends":
        oracle.rng_reset(); oracle.expander_init_store(trs)
        hb.upload_graphs(trs, bm.graphs(oracle, trs))
    else:
        hb.rng_reset(); hb.expander_init_store(trs)
    d = hb.fill_splitmix(N, 100 + logN + K)
    x = splitmix_field(logN, 7)
    c = hb.commit_standard((d, N), K, trs, 1)
    if change is not None:
        v = hb.to_host(d, (2,), np.uint64, offset=16 * change)
        v[0] ^= np.uint64(1)
        hb._chk(hb.lib.hobbit_memcpy_h2d(hb.ctx, c_vp(d.ptr + 16 * change), _p(v), c_sz(16)))
    libc.srandom(seed)
    t0 = time.perf_counter()
    o = hb.open_standard((d, N), c, x, queries, want_paths=False)
    t_open = time.perf_counter() - t0
    c.free()
    d_aggr, aggr = device_aggregate(hb, d, N, K, x)
    d.free()
    keep = [d_aggr]
    if where == "oracle_ends":
        evalC, evalA = oracle_evaluators(oracle, aggr, trs)
    else:
        evalC, evalA, d_T = device_evaluators(hb, d_aggr, M, trs)
        keep.append(d_T)
    print("(2^%d, %d, %d): trs %d, open_standard %.2f s" % (logN, K, queries, trs, t_open))
    return o, x, trs, evalC, evalA, keep


def verify_everything(o, x, K, trs, evalC, evalA):
    ov.verify_open(o, x, K, trs, lambda pc, pa: (fi(evalC(pc)), fi(evalA(pa))))
    pc, _, pf = ov.open_points(o, x, K, trs)
    ov.verify_shockwave(o["sp_c"], pc, 32, ov.matrix_end(evalC, pc, 32), "sp_c")
    ov.verify_shockwave(o["sp_f"], pf, 32, ov.matrix_end(evalA, pf, 32), "sp_f")


SHAPES = [
    (16, 4, 300, "oracle_ends"),        # the smallest
    (18, 32, 5900, "oracle_ends"),      # trs = 4, the identity code; sp_f (width 256) without a WHIR proof, sp_c (width 512) with one
    (20, 4, 1, "oracle_ends"),          # one query, two queries,
    (20, 4, 2, "oracle_ends"),
    (20, 4, 20000, "oracle_ends"),      # ... and about 190 overwritten positions
    (24, 32, 5900, "oracle_ends"),      # the largest transcript-pinned K = 32 shape
    (26, 32, 5900, "oracle_ends"),      # the smallest shape whose tensor passes 2^32 bytes; beyond any K = 32 oracle run
    (24, 2, 5900, "device_ends"),       # trs = 4096, the benchmark's code: queries land in the unwritten zero rows
    (28, 32, 5900, "device_ends"),      # the benchmark's shape
]


@pytest.mark.parametrize("logN,K,queries,where", SHAPES, ids=["2e%d-K%d-q%d-%s" % s for s in SHAPES])
def test_the_devices_opening_verifies(hb, oracle, logN, K, queries, where):
    o, x, trs, evalC, evalA, keep = commit_and_open(hb, oracle, logN, K, queries, where, seed=1000 + logN)
    assert o["checks"].tolist() == [1, 1, 1]
    distinct = len(ov.last_writes(o["I"], COLS))
    if (logN, queries) == (20, 20000):
        assert 100 <= queries - distinct <= 300                # 20000 queries in 2^20 positions: about 190 are overwritten
    if (logN, K) == (18, 32):
        assert trs == 4 and int(o["sp_f"]["iters"][0]) == 0 and int(o["sp_c"]["iters"][0]) >= 1
    if trs == 4096:
        rows = o["I"][:, 1]
        tail = np.flatnonzero(rows >= 7 * trs // 4)             # the codeword of 4096 has 1.72 * 4096 entries: these rows are never written
        assert len(tail) and not o["reply"][tail].any()
    verify_everything(o, x, K, trs, evalC, evalA)
    for b in keep:
        b.free()


def test_the_device_opens_another_polynomial_and_the_verifier_rejects_it(hb, oracle):
    """(2^20, 32): committed, then one bit of one coefficient changed, then opened over the committed tensor.  The device's checks read
    [1, 1, 1]; the verifier rejects at P3's claim.  The same opening without the change is accepted"""
    logN, K = 20, 32
    o, x, trs, evalC, evalA, keep = commit_and_open(hb, oracle, logN, K, 5900, "oracle_ends", seed=777, change=(1 << logN) // 3)
    assert o["checks"].tolist() == [1, 1, 1]
    with pytest.raises(Rejected) as e:
        verify_everything(o, x, K, trs, evalC, evalA)
    assert e.value.relation == ov.P3_CLAIM
    good, x2, _, evalC, evalA, keep2 = commit_and_open(hb, oracle, logN, K, 5900, "oracle_ends", seed=777)
    assert np.array_equal(x, x2) and np.array_equal(good["I"], o["I"]) and np.array_equal(good["reply"], o["reply"])
    verify_everything(good, x, K, trs, evalC, evalA)
    for b in keep + keep2:
        b.free()


@pytest.mark.parametrize("logN,k", [(10, 4), (14, 32), (18, 64)])
def test_the_devices_shockwave_proof_verifies(hb, oracle, logN, k):
    """hobbit_shockwave_commit + hobbit_shockwave_prove alone; the end from the host matrix"""
    m = splitmix_field(1 << logN, 30 + logN); x = splitmix_field(logN, 31)
    enc, lv = hb.shockwave_commit(m, k)
    libc.srandom(9)
    sp = hb.shockwave_prove(m, enc, k, x, lv)
    ov.verify_shockwave(sp, x, k, ov.matrix_end(lambda p: oracle.evaluate_vector(m, p), x, k))
    assert (int(sp["iters"][0]) > 0) == ((1 << logN) // k > 256)
    bad = dict(sp); bad["reply"] = sp["reply"].copy()
    last = ov.last_columns(sp["I"])[int(sp["I"][0])]
    bad["reply"][last, k - 1, 1] ^= np.uint64(1)
    with pytest.raises(Rejected) as e:
        ov.verify_shockwave(bad, x, k, ov.matrix_end(lambda p: oracle.evaluate_vector(m, p), x, k))
    assert e.value.relation == ov.SP_P1_CLAIM
