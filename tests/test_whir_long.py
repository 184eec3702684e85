"""WHIR proofs to 2^26 coefficients (include/hobbit_whir.h): hobbit_whir_ood, hobbit_whir_prove_any, the mirror's whir_commit / _whir_prove
and `host/test_pc whir <logN>`.  Everything is bit for bit.

  1. hobbit_whir_ood alone against the oracle's precompute_beta and field operations: every v from 1 to 14 (the low half of a table has
     min(v, 4) variables: v below, at and above it, one row, rows that do not fill a wave, more than one workgroup) x R in {1, 7, 100}; beta
     starts non-zero; the points include the all-zero, all-one and all-(p - 1) ones, the polynomial runs of p - 1.  One back-to-back pair.
  2. whir_prove_any against the oracle at logN = 9, 12, 13, 17, 20 (one size per iteration class and both edges of the first), against
     hobbit_whir_prove at 21 and 24, the refusals, and 2^25 / 2^26 against tests/golden/whir_long.npz (scripts/gen_whir_long_golden.py:
     the oracle takes minutes there).
  3. the driver as a child process against the same run through the ABI.
  4. (no GPU) WHIR_SYMBOLS against the header and the library; the two host generators behind the fixture; the lazy sums of
     csrc/hobbit_whir_acc.hpp against 128-bit arithmetic.
"""
import ctypes
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
P = (1 << 61) - 1
libc = ctypes.CDLL(None)
SEED_POLY, SEED_X, SRANDOM = 9100, 9200, 7                  # scripts/gen_whir_long_golden.py
KEYS = ("iters", "poly", "a", "roots", "scal", "checks", "qn", "qidx", "qreply", "qpaths", "final_pb")


def _mod():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def same(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


# ---- 4. no GPU -------------------------------------------------------------------------------------------------------------------------
def test_whir_symbols_match_the_header_and_the_library():
    mod = _mod()
    with open(os.path.join(ROOT, "include", "hobbit_whir.h")) as f:
        text = f.read()
    declared = re.findall(r"^int (hobbit_[a-z0-9_]+)\(", text, re.M)
    assert sorted(declared) == sorted(mod.WHIR_SYMBOLS) and len(set(declared)) == len(declared)
    assert '#include "hobbit_hip.h"' in text
    with open(os.path.join(ROOT, "include", "hobbit_hip.h")) as f:
        first = f.read()
    for s in mod.WHIR_SYMBOLS:
        assert s + "(" not in first and s not in mod.ABI_SYMBOLS and s not in mod.PARITY_SYMBOLS
    lib = mod.load_library()
    assert [s for s in mod.WHIR_SYMBOLS if not hasattr(lib, s)] == []


def test_the_two_host_generators_agree():
    """pins the two HOST generators against each other, not the device fill: the fixture's polynomial is pyoracle.splitmix_field, and the
    package's splitmix_field is what hobbit_fill_splitmix is documented to reproduce.  The device fill itself is compared with
    pyoracle.splitmix_field on the GPU, on the first 2^12 elements, inside test_whir_prove_any_long."""
    for logN in (25, 26):
        assert np.array_equal(_mod().splitmix_field(1 << 12, SEED_POLY + logN), splitmix_field(1 << 12, SEED_POLY + logN))


def test_lazy_sums_against_128_bit_arithmetic(tmp_path):
    """csrc/hobbit_whir_acc.hpp is plain C++: tests/whir_acc_check.cpp, built with g++, compares 200 000 lazy sums of 1 ... 300 products
    (random and edge operands, runs of (p - 1)(p - 1)) with fadd(fmul()) on the host's 128-bit path, and one sum of 2^20 largest products
    (the carry counts)"""
    exe = str(tmp_path / "whir_acc_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "whir_acc_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "0 bad" in p.stdout, (p.returncode, p.stdout[-300:], p.stderr[-300:])


# ---- 1. the out-of-domain step -----------------------------------------------------------------------------------------------------------
def field_sum(oracle, v):
    v = np.ascontiguousarray(v, np.uint64).reshape(-1, 2)
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.concatenate([v, np.zeros((1, 2), np.uint64)])
        v = oracle.f_add(v[: v.shape[0] // 2], v[v.shape[0] // 2:])
    return v[0]


def ood_inputs(v, R, seed):
    n = 1 << v
    poly, beta = splitmix_field(n, seed), splitmix_field(n, seed + 1)
    poly[::3] = P - 1                                       # the largest products
    if n >= 8:
        poly[5] = 0
    z = splitmix_field(R * v, seed + 2).reshape(R, v, 2).copy(); pw = splitmix_field(R, seed + 3)
    if R >= 7:
        z[0] = 0; z[1] = 0; z[1, :, 0] = 1; z[2] = P - 1; pw[3] = (P - 1, P - 1)
    return poly, beta, z, pw


def ood_reference(oracle, poly, beta, z, pw):
    y = np.zeros((z.shape[0], 2), np.uint64); b = beta.copy()
    for i in range(z.shape[0]):
        eq = oracle.precompute_beta(z[i])
        y[i] = field_sum(oracle, oracle.f_mul(eq, poly))
        b = oracle.f_add(b, oracle.f_mul(np.repeat(pw[i].reshape(1, 2), eq.shape[0], 0), eq))
    return y, b


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 7, 100])
@pytest.mark.parametrize("v", list(range(1, 15)))
def test_whir_ood_against_the_oracle(hb, oracle, v, R):
    poly, beta, z, pw = ood_inputs(v, R, 100 * v + R)
    want_y, want_b = ood_reference(oracle, poly, beta, z, pw)
    y, b = hb.whir_ood(poly, beta, z, pw)
    assert np.array_equal(y, want_y), "y"
    assert np.array_equal(b, want_b), "beta"


@pytest.mark.gpu
def test_whir_ood_grid_stride(hb, oracle):
    """v = 23: 2^19 rows, twice what the 1024 workgroups of k_whir_ood_y cover in one trip, and four trips of k_whir_ood_beta's loop (no
    shape a proof passes gets there: its first step has v <= 22).  R = 2: one slice of two points"""
    poly, beta, z, pw = ood_inputs(23, 2, 2302)
    want_y, want_b = ood_reference(oracle, poly, beta, z, pw)
    y, b = hb.whir_ood(poly, beta, z, pw)
    assert np.array_equal(y, want_y), "y"
    assert np.array_equal(b, want_b), "beta"


@pytest.mark.gpu
def test_whir_ood_refusals(hb):
    d = hb.to_device(splitmix_field(16, 1)); h = splitmix_field(200, 2)
    for v, R in ((0, 4), (27, 4), (4, 0), (4, 129)):
        assert hb.lib.hobbit_whir_ood(hb.ctx, d.ptr, d.ptr, v, vp(h), vp(h), R, d.ptr) < 0, (v, R)
        assert b"whir_ood" in hb.lib.hobbit_last_error(hb.ctx)
    assert hb.lib.hobbit_whir_ood(hb.ctx, d.ptr, d.ptr, 4, None, vp(h), 4, d.ptr) < 0


@pytest.mark.gpu
def test_whir_ood_back_to_back_pair(hb):
    """two calls queued behind each other (behind a backlog of unrelated products on the same stream), the h_* inputs overwritten the moment
    each call returns: both results equal those of the two calls run alone with a sync after each"""
    shapes = ((9, 7, 5001), (13, 100, 5002))

    def run(alone):
        bufs, ins = [], []
        for v, R, seed in shapes:
            poly, beta, z, pw = ood_inputs(v, R, seed)
            bufs.append((hb.to_device(poly), hb.to_device(beta), hb.to_device(np.full((R, 2), 0xC3C3, np.uint64))))
            ins.append((np.ascontiguousarray(z), np.ascontiguousarray(pw)))
        hb.sync()
        if not alone:
            a, b = hb.fill_splitmix(1 << 22, 1), hb.fill_splitmix(1 << 22, 2); o = hb.alloc(16 << 22)
            for _ in range(100):
                hb._chk(hb.lib.hobbit_f_binop(hb.ctx, 2, a.ptr, b.ptr, o.ptr, 1 << 22))
        for (v, R, _), (dp, db, dy), (z, pw) in zip(shapes, bufs, ins):
            hb._chk(hb.lib.hobbit_whir_ood(hb.ctx, dp.ptr, db.ptr, v, vp(z), vp(pw), R, dy.ptr))
            z.view(np.uint8)[...] = 0xEE; pw.view(np.uint8)[...] = 0xEE
            if alone:
                hb.sync()
        hb.sync()
        return [(hb.to_host(dy, (R, 2), np.uint64), hb.to_host(db, (1 << v, 2), np.uint64)) for (v, R, _), (dp, db, dy) in zip(shapes, bufs)]
    want, got = run(True), run(False)
    assert not np.array_equal(want[0][0], want[1][0][:7])
    for k in range(2):
        assert np.array_equal(got[k][0], want[k][0]), "y of call %d" % k
        assert np.array_equal(got[k][1], want[k][1]), "beta of call %d" % k


# ---- 2. the proof --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("logN,iters", [(9, 2), (12, 2), (13, 3), (17, 4), (20, 4)])
def test_whir_prove_any_against_the_oracle(hb, oracle, logN, iters):
    p, x = splitmix_field(1 << logN, 1), splitmix_field(logN, 2)
    libc.srandom(7); want = oracle.whir_prove(p, x); after_oracle = libc.rand()
    libc.srandom(7); got = hb.whir_prove_any(p, x); after_device = libc.rand()
    assert want["checks"].tolist() == [1, 1] and got["checks"].tolist() == [1, 1]
    assert int(want["iters"][0]) == iters
    same(got, want, "logN=%d" % logN)
    assert after_device == after_oracle, "the libc stream is left at another point"


@pytest.mark.gpu
@pytest.mark.parametrize("logN", [21, 24])
def test_whir_prove_any_against_whir_prove(hb, logN):
    N = 1 << logN
    d = hb.fill_splitmix(N, 31 + logN); x = splitmix_field(logN, 32)
    com, lv = hb.alloc(32 * N), hb.alloc(32 * N)
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N, com.ptr, lv.ptr))
    libc.srandom(11); want = hb.whir_prove((d, N), x, com, lv); after_a = libc.rand()
    libc.srandom(11); got = hb.whir_prove_any((d, N), x, com, lv); after_b = libc.rand()
    assert want["checks"].tolist() == [1, 1] and int(want["iters"][0]) == 5
    same(got, want, "logN=%d" % logN)
    assert after_a == after_b
    for b in (d, com, lv):
        b.free()


def whir_out(logN=27):
    """a hobbit_whir_out over real host buffers, as Hobbit._whir_prove builds it; returns (struct, the arrays that back it)"""
    bufs = dict(qpoly=np.zeros((logN + 8, 3, 2), np.uint64), a=np.zeros((logN + 8, 2), np.uint64), fri_roots=np.zeros((logN, 32), np.uint8),
                scal=np.zeros((2, 2), np.uint64), checks=np.zeros(2, np.int32), iters=np.zeros(1, np.int32))
    bufs.update(_mod().Hobbit._wq_buffers())
    names = ("qpoly", "a", "fri_roots", "scal", "checks", "iters") + _mod().Hobbit._WQ_NAMES

    class Out(ctypes.Structure):
        _fields_ = [(n, ctypes.c_void_p) for n in names]
    return Out(*[bufs[n].ctypes.data for n in names]), bufs


@pytest.mark.gpu
def test_whir_prove_any_refusals(hb):
    """2^8 (where the reference itself fails), 2^27, no power of two, zero, each with every other argument valid: refused for its size
    before anything is drawn or launched.  Separately a NULL out with a valid N: refused likewise, before the plan draws.  The same
    arguments with N = 2^9 are then accepted, so nothing but N decided the refusals."""
    N0 = 1 << 9
    d = hb.to_device(splitmix_field(N0, 1)); x = splitmix_field(27, 2)
    com, lv = hb.alloc(32 * N0), hb.alloc(32 * N0)
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N0, com.ptr, lv.ptr))
    o, bufs = whir_out()
    hb.sync(); hb.profile(True); hb.profile_reset()
    try:
        libc.srandom(5); before = libc.rand(); libc.srandom(5)
        for N in (1 << 8, 1 << 27, 1000, 0):
            assert hb.lib.hobbit_whir_prove_any(hb.ctx, d.ptr, N, com.ptr, lv.ptr, vp(x), ctypes.byref(o)) < 0, N
            assert b"whir_prove_any: N must be a power of two in [2^9, 2^26]" in hb.lib.hobbit_last_error(hb.ctx), N
        assert hb.lib.hobbit_whir_prove_any(hb.ctx, d.ptr, N0, com.ptr, lv.ptr, vp(x), None) < 0
        assert b"whir_prove_any: NULL out" in hb.lib.hobbit_last_error(hb.ctx)
        assert libc.rand() == before, "a refused call drew from the libc generator"
        hb.sync()
        assert not hb.profile_report(), "a refused call launched %s" % sorted(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()
    libc.srandom(5)
    hb._chk(hb.lib.hobbit_whir_prove_any(hb.ctx, d.ptr, N0, com.ptr, lv.ptr, vp(x), ctypes.byref(o)))
    assert bufs["checks"].tolist() == [1, 1] and int(bufs["iters"][0]) == 2 and libc.rand() != before


@pytest.mark.gpu
@pytest.mark.parametrize("logN", [25, 26])
def test_whir_prove_any_long(hb, logN):
    """2^25: the first six-iteration size and the first three-factor FRI transform; 2^26: the upper edge (path depth 25, remaining = 4)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "whir_long.npz"))
    G = lambda k: g["%d_%s" % (logN, k)]
    N = 1 << logN
    d = hb.fill_splitmix(N, SEED_POLY + logN); x = splitmix_field(logN, SEED_X + logN)
    assert np.array_equal(hb.to_host(d, (1 << 12, 2), np.uint64), splitmix_field(1 << 12, SEED_POLY + logN))
    com, lv = hb.alloc(32 * N), hb.alloc(32 * N)
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N, com.ptr, lv.ptr))
    assert np.array_equal(hb.to_host(lv, (32,), np.uint8, offset=32 * (N - 2)), G("commit_root")), "whir_commit root"
    libc.srandom(SRANDOM); got = hb.whir_prove_any((d, N), x, com, lv); after = libc.rand()
    assert int(got["iters"][0]) == 6 and got["checks"].tolist() == [1, 1]
    assert int(got["final_pb"].shape[0]) == 2 * (N >> 24)
    for k in ("iters", "poly", "a", "roots", "scal", "checks", "qn", "qidx", "final_pb"):
        assert got[k].shape == G(k).shape and np.array_equal(got[k], G(k)), k
    assert after == int(G("rand_after")[0]), "the libc stream is left at another point"
    # the first path of every round in full, then everything by digest
    off, firsts = 0, []
    for t, n in enumerate(got["qn"]):
        depth = ((2 * N) >> t).bit_length() - 1 - 2
        if n:
            firsts.append(got["qpaths"][off:off + 32 * depth])
        off += int(n) * 32 * depth
    assert np.array_equal(np.concatenate(firsts), G("first_paths")), "first path of a round"
    assert hashlib.sha256(np.ascontiguousarray(got["qreply"]).tobytes()).digest() == bytes(G("qreply_sha256")), "qreply"
    assert hashlib.sha256(np.ascontiguousarray(got["qpaths"]).tobytes()).digest() == bytes(G("qpaths_sha256")), "qpaths"
    for b in (d, com, lv):
        b.free()


# ---- 3. mirror and driver --------------------------------------------------------------------------------------------------------------
def whir_ps(res, N):
    """ps of one _whir_prove (src/Virgo.cpp:557, 262, 643) in the reference's order of accumulation, as the mirror's whir_ps"""
    ps, q, it = 0.0, 0, int(res["iters"][0])
    for t in range(1, it + 1):
        for _ in range(4):
            ps += 3 * 16 / 1024.0
        size = (2 * N) >> (t - 1)
        n = int(res["qn"][t - 1])
        if t == it:
            ps += (N >> (4 * it)) * 2 * 16 / 1024.0
        ps += 16.0 * n * 16 / 1024.0
        for p in path_ps_terms(size // 4, (size // 4).bit_length() - 1, res["qidx"][q:q + n]):
            ps += p
        q += n
    return ps


def path_ps_terms(n_leaves, depth, pos):
    """verify_claim_opt_blake's accounting (src/merkle_tree.cpp:326-361), term by term: the mirror adds each 32 B to the running sum"""
    visited = set()
    for p in pos:
        pe = n_leaves + int(p)
        for _ in range(depth):
            if (pe ^ 1) in visited:
                break
            visited.add(pe ^ 1); pe //= 2; visited.add(pe)
            yield 32.0 / 1024.0


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [14, 20])
def test_host_test_pc_whir(hb, logn):
    """`host/test_pc whir <logN>` in a child process: root and ps equal those of the same run through the ABI from the same libc state"""
    exe = os.path.join(PKG, "host", "test_pc")
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "whir", str(logn)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    N = 1 << logn
    libc.srandom(1)                                         # a fresh process: test_PC draws the polynomial, then x, then the proof's draws
    poly = hb.generate_randomness(N)
    _, lv = hb.whir_commit(poly)
    x = hb.generate_randomness(logn)
    res = hb.whir_prove_any(poly, x)
    assert res["checks"].tolist() == [1, 1]
    m = re.search(r"^root ([0-9a-f]{64})$", p.stdout, re.M)
    assert m and m.group(1) == bytes(lv[-1]).hex(), p.stdout[-500:]
    assert re.search(r"^Commit time: \S+ seconds$", p.stdout, re.M)
    m = re.search(r"^PC Total: pt = (\S+), ps = (\S+), vt = (\S+)$", p.stdout, re.M)
    assert m, p.stdout[-500:]
    assert m.group(2) == "%f" % whir_ps(res, N), (m.group(2), whir_ps(res, N))
