"""Codes of 2^21: the long forms of the Braking base baseline (include/hobbit_longcodes.h) and what was lifted beneath them -- the finalize and
the rows-innermost encode at n = 2^21, the parity matrix at P = 2^26, the nested WHIR proof of hobbit_shockwave_prove at a width of 2^25.

Neither the oracle nor tests/parity_model.py can run an opening at P = 2^26, so the opening at 2^21 rests on independent checks:
  * the verifier's round test of every sumcheck in the output, on the host in Python integers (check_rounds / check_tree below; the CPU tests
    pin them with the oracle's own sumchecks and tree, and the old-ground GPU test runs them on an opening that equals the existing call's);
  * P2's claimed sum against eq(r2)^T A(r1) computed without the access lists, by the device's hobbit_parity_matrix and by the oracle;
  * the nested WHIR proofs against a direct hobbit_whir_commit + hobbit_whir_prove_any of the same aggregate at the same libc position.
The smallest shapes that reach the new ground: n = 2^21 at rows = 1 and 4, and (N, K) = (2^23, 4).  The graphs of 2^21 are drawn once
(rng_reset, expander_init_store(2^21): 2 s) and shared; the codewords of the four rows of the polynomial are encoded once by the oracle.
"""
import ctypes
import os
import re
import subprocess
import time

import numpy as np
import pytest

import brakingbase_model as bm
import commit_refs
from open_verifier import ONE, ZERO, check_rounds, claim, ev, fadd, fi, fmul, fsub
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
P = (1 << 61) - 1
N21 = 1 << 21
libc = ctypes.CDLL(None)
libc.random.restype = ctypes.c_long
libc.initstate.restype = ctypes.c_void_p
libc.initstate.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
libc.setstate.restype = ctypes.c_void_p
libc.setstate.argtypes = [ctypes.c_void_p]


def _mod():
    from __graft_entry__ import load_package
    return load_package()


# ---- F_{p^2} in Python integers and the verifier's round test: tests/open_verifier.py ------------------------------------------------------------------


def check_tree(t, vectors, what):
    """prove_multiplication_tree_new's layers: layer k is a cubic sumcheck of log2(vectors) + k rounds (in1, in2, eq); its claim is the line
    through the layer above's two final values at that layer's closing challenge"""
    layers = int(t["layers"][0]); rl = vectors.bit_length() - 1
    assert layers >= 1 and rl >= 1, what
    at, want = 0, None
    for k in range(layers):
        q, r = t["poly"][at:at + rl], t["r"][at:at + rl]
        got = check_rounds(q, r, t["vr"][k], "%s layer %d" % (what, k))
        if want is not None:
            assert got == want, "%s: claim of layer %d" % (what, k)
        f = fi(t["fin"][k])
        want = fadd(fmul(fi(t["vr"][k][0]), fsub(ONE, f)), fmul(fi(t["vr"][k][1]), f))
        at += rl; rl += 1
    assert fi(t["final_eval"]) == want, what + ": final evaluation"
    return layers


def check_shockwave(sp, what):
    """P1 / P2 of one shockwave_prove and its WHIR checks; prove_fft's last challenge is popped from r2 (src/sumcheck.cpp:2985) but still lies
    in the buffer behind the trimmed view"""
    check_rounds(sp["q1"], sp["r1"], sp["vr1"], what + " P1")
    r2 = sp["r2"].base if sp["r2"].base is not None and len(sp["r2"].base) == len(sp["q2"]) else sp["r2"]
    assert len(r2) == len(sp["q2"]), what + ": the popped challenge is not behind the view"
    check_rounds(sp["q2"], r2, sp["vr2"], what + " P2")
    if int(sp["iters"][0]):
        assert sp["wchecks"].tolist() == [1, 1], what + " WHIR"


def check_opening(o, K, what):
    """every sumcheck of one hobbit_brakingbase_open[_any] output; returns P2's claimed sum"""
    assert o["checks"].tolist() == [1, 1], what
    assert check_rounds(o["p1"]["poly"], o["p1"]["r"], o["p1"]["vr"], what + " P1") == ZERO, what + ": P1's claimed sum is not zero"
    par = o["parity"]
    check_tree(par["t1"], 4, what + " tree 1"); check_tree(par["t2"], 4, what + " tree 2")
    p2 = check_rounds(par["p2"]["poly"], par["p2"]["r"], par["p2"]["vr"], what + " P2")
    check_rounds(par["p3"]["poly"], par["p3"]["r"], par["p3"]["vr"], what + " P3")
    check_rounds(par["p4"]["poly"], par["p4"]["r"], par["p4"]["vr"], what + " P4")
    check_shockwave(par["sp_p"], what + " sp_p"); check_shockwave(par["sp_w"], what + " sp_w"); check_shockwave(o["sp_c"], what + " sp_c")
    return p2


# ---- the libc generator as an object: seeded, snapshotted and restored from outside -----------------------------------------------------------------
class LibcStream:
    """random() / rand() on a state array of ours (the default generator's kind: 128 bytes).  setstate() to another array writes the position
    into ours, so a copy of the array is a snapshot of the stream"""

    def __init__(self, seed):
        self.buf = ctypes.create_string_buffer(128); self.side = ctypes.create_string_buffer(128)
        self.prev = libc.initstate(1, self.side, 128)           # the generator in use before: put back by close()
        libc.initstate(seed, self.buf, 128)

    def snapshot(self):
        libc.setstate(self.side)
        data = self.buf.raw
        libc.setstate(self.buf)
        return data

    def restore(self, data, skip=0):
        libc.setstate(self.side)
        ctypes.memmove(self.buf, data, 128)
        libc.setstate(self.buf)
        for _ in range(skip):
            libc.random()

    def find(self, data, values, limit=1 << 22):
        """how many draws after the snapshot the run `values` begins"""
        self.restore(data)
        win = [libc.random() for _ in range(len(values))]
        for d in range(limit):
            if win == values:
                return d
            win.pop(0); win.append(libc.random())
        raise AssertionError("the draws were not found on the stream")

    def close(self):
        if self.prev:
            libc.setstate(self.prev)
            self.prev = None


def same(a, b, what):
    if isinstance(b, dict):
        assert sorted(a) == sorted(b), what
        for k in b:
            if k != "stage_ms":
                same(a[k], b[k], what + "/" + k)
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


# ---- CPU: the helpers above against the oracle ----------------------------------------------------------------------------------------------------------
def test_field_helpers_are_the_oracles(oracle):
    a, b = pyoracle.splitmix_field(64, 1), pyoracle.splitmix_field(64, 2)
    m, s, d = oracle.f_mul(a, b), oracle.f_add(a, b), oracle.f_sub(a, b)
    for i in range(64):
        assert fmul(fi(a[i]), fi(b[i])) == fi(m[i]) and fadd(fi(a[i]), fi(b[i])) == fi(s[i]) and fsub(fi(a[i]), fi(b[i])) == fi(d[i])


@pytest.mark.parametrize("n", [2, 8, 1 << 10])
def test_round_tests_accept_the_oracles_sumchecks_and_reject_a_changed_one(oracle, n):
    v = [pyoracle.splitmix_field(n, 10 + i) for i in range(3)]
    pr = np.array([33, 0], np.uint64)
    p2 = oracle.sumcheck2(v[0], v[1], pr); p3 = oracle.sumcheck3(v[0], v[1], v[2], pr)
    tot2 = tot3 = ZERO
    for i in range(n):
        tot2 = fadd(tot2, fmul(fi(v[0][i]), fi(v[1][i]))); tot3 = fadd(tot3, fmul(fmul(fi(v[0][i]), fi(v[1][i])), fi(v[2][i])))
    assert check_rounds(p2["poly"], p2["r"], p2["vr"], "sumcheck2") == tot2
    assert check_rounds(p3["poly"], p3["r"], p3["vr"], "sumcheck3") == tot3
    for p in (p2, p3):
        bad = p["poly"].copy(); bad[-1, 0, 0] ^= np.uint64(1)
        with pytest.raises(AssertionError):
            check_rounds(bad, p["r"], p["vr"], "changed")


def test_tree_test_accepts_the_oracles_tree_and_rejects_a_changed_one(oracle):
    libc.srandom(4)
    t = oracle.mul_tree(pyoracle.splitmix_field(4 * 64, 3).reshape(4, 64, 2), np.array([21, 0], np.uint64))
    assert check_tree(t, 4, "tree") == 6
    bad = dict(t); bad["vr"] = t["vr"].copy(); bad["vr"][2, 0, 0] ^= np.uint64(1)
    with pytest.raises(AssertionError):
        check_tree(bad, 4, "changed")


def test_libc_stream_snapshots():
    s = LibcStream(11)
    try:
        snap = s.snapshot()
        a = [libc.random() for _ in range(40)]
        s.restore(snap)
        assert [libc.random() for _ in range(40)] == a
        s.restore(snap, skip=7)
        assert [libc.rand() for _ in range(5)] == a[7:12]
        assert s.find(snap, a[30:34]) == 30
    finally:
        s.close()


# ---- CPU: the header and its symbols --------------------------------------------------------------------------------------------------------------------
ASYNC = {"hobbit_brakingbase_commit_any"}          # hobbit_brakingbase_commit's body: its stream test is tests/test_brakingbase.py's
HOST_RETURNING = {"hobbit_brakingbase_open_any"}
EXEMPT = {"hobbit_brakingbase_shape_any": "host only"}


def declared(header="hobbit_longcodes.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    from __graft_entry__ import build_hip
    build_hip()
    mod = _mod()
    lib = mod.load_library()
    decl = declared()
    assert len(decl) == 3 and sorted(mod.LONGCODES_SYMBOLS) == decl
    for s in decl:
        assert hasattr(lib, s), "missing export " + s
        assert getattr(lib, s).argtypes is not None, "no prototype bound for " + s
    for other in (mod.ABI_SYMBOLS, mod.PARITY_SYMBOLS, mod.PARITY_LISTS_SYMBOLS, mod.WHIR_SYMBOLS, mod.BRAKINGBASE_SYMBOLS, mod.ORION_SYMBOLS):
        assert not set(decl) & set(other)
    for header in ("hobbit_hip.h", "hobbit_parity.h", "hobbit_parity_lists.h", "hobbit_whir.h", "hobbit_brakingbase.h", "hobbit_orion.h"):
        assert not [s for s in declared(header) if s.endswith("_any") and "brakingbase" in s], header
    for meth in ("brakingbase_shape_any", "brakingbase_commit_any", "brakingbase_open_any"):
        assert callable(getattr(mod.Hobbit, meth))


def test_every_export_is_classified():
    sets = {"ASYNC": ASYNC, "HOST_RETURNING": HOST_RETURNING, "EXEMPT": set(EXEMPT)}
    names = set(declared())
    for n in sorted(names):
        assert len([k for k, s in sets.items() if n in s]) == 1, n
    for k, s in sets.items():
        assert not (s - names), (k, sorted(s - names))


def test_shape_any():
    """the old range as hobbit_brakingbase_shape gives it, (2^23, 4) and (2^28, 128) beyond it; (2^28, 64) is refused (trs = 2^22: the fallback
    this library ships with), and so are trs = 2^23, K = 2, K = 1024 and what is no power of two"""
    from __graft_entry__ import build_hip
    build_hip()
    hb = _mod().Hobbit
    for logn in range(9, 30):
        for K in (4, 8, 64, 128, 256, 512):
            N = 1 << logn
            try:
                old = hb.brakingbase_shape(N, K)
            except _mod().HobbitError:
                old = None
            if old is not None:
                assert hb.brakingbase_shape_any(N, K) == old == N // K
            elif N // K == N21:
                assert hb.brakingbase_shape_any(N, K) == N21
    assert hb.brakingbase_shape_any(1 << 23, 4) == N21 and hb.brakingbase_shape_any(1 << 28, 128) == N21
    assert hb.brakingbase_shape_any(1 << 9, 4) == 128 and hb.brakingbase_shape_any(1 << 28, 256) == 1 << 20
    for N, K in ((1 << 28, 64), (1 << 25, 4), (1 << 24, 4), (1 << 22, 2), (1 << 30, 1024), (3 << 21, 4), (1 << 23, 6), (1 << 8, 4), (0, 4), (1 << 23, 0)):
        with pytest.raises(_mod().HobbitError):
            hb.brakingbase_shape_any(N, K)


def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


def test_host_test_pc_brakingbase_any_refusals():
    """a bad shape ends with status 255 before anything is drawn or any device is opened; (2^28, 64) says why"""
    from __graft_entry__ import build_hip, build_host
    build_hip(); build_host()
    for args in (("brakingbase_any", 30, 64), ("brakingbase_any", 10, 256), ("brakingbase_any", 28, 64), ("brakingbase_any", 20, 3), ("brakingbase_any", 22, 2),
                 ("brakingbase_any", 0, 4)):
        p = _test_pc(args, 120)
        assert p.returncode == 255 and "Error: Braking base" in p.stdout and "root" not in p.stdout, (args, p.returncode, p.stdout[-300:])
    out = _test_pc(("brakingbase_any", 28, 64), 120).stdout
    assert "longer than 2^21" in out and "2^31" in out, out[-300:]


# ---- the device -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)
    yield h
    h.close()


_ORC_N = [None]


def oracle_graphs(orc, n):
    """the oracle's graphs of n, from rng_reset: drawn again only when another n (or another module) has replaced them"""
    if _ORC_N[0] != n:
        orc.rng_reset(); orc.expander_init_store(n)
        _ORC_N[0] = n


def device_graphs(hb, orc, n):
    oracle_graphs(orc, n)
    return hb.upload_graphs(n, bm.graphs(orc, n))


@pytest.fixture(scope="module")
def code21(hb, oracle):
    """the graphs of 2^21 drawn by the oracle and finalized on the device; the finalize's host time is printed (it is reported, not bounded)"""
    oracle_graphs(oracle, N21)
    levels = bm.graphs(oracle, N21)
    hb._chk(hb.lib.hobbit_graph_reset(hb.ctx))
    for (dep, kind), g in levels.items():
        nbr = np.ascontiguousarray(g["nbr"], np.int64); w = np.ascontiguousarray(g["w"], np.uint64)
        hb._chk(hb.lib.hobbit_graph_upload(hb.ctx, dep, kind, g["L"], g["R"], g["degree"], nbr.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p)))
    ln = ctypes.c_longlong()
    t0 = time.perf_counter()
    hb._chk(hb.lib.hobbit_graph_finalize(hb.ctx, ctypes.c_longlong(N21), ctypes.byref(ln)))
    print("hobbit_graph_finalize(2^21): %.2f s on the host, codeword length %d" % (time.perf_counter() - t0, ln.value))
    return dict(n=N21, len=ln.value)


@pytest.fixture(scope="module")
def rows21(oracle, code21):
    """the polynomial of (2^23, 4) and the oracle's codewords of its four rows"""
    oracle_graphs(oracle, N21)
    poly = pyoracle.splitmix_field(1 << 23, 7)
    cw = [oracle.encode_monolithic(poly[i * N21:(i + 1) * N21]) for i in range(4)]
    assert all(c[1] == code21["len"] for c in cw)
    return dict(poly=poly, T=np.stack([c[0] for c in cw]))


@pytest.mark.gpu
@pytest.mark.parametrize("logn,K", [(16, 64), (14, 128)])
def test_any_gives_the_existing_calls_bits(hb, oracle, logn, K):
    """on old ground the long forms are the existing calls: root and levels, every output buffer of the opening (nested transcripts included)
    and the position of the libc stream afterwards; the round tests of this file hold on that opening"""
    N = 1 << logn; trs = N // K
    device_graphs(hb, oracle, trs)
    poly = pyoracle.splitmix_field(N, 40 + K); x = pyoracle.splitmix_field(logn, 41)
    a, b = hb.brakingbase_commit(poly, K), hb.brakingbase_commit_any(poly, K)
    assert np.array_equal(a.root(), b.root()) and np.array_equal(a.levels(), b.levels())
    assert (a.N, a.K, a.trs, a.len) == (b.N, b.K, b.trs, b.len)
    s = LibcStream(123)
    try:
        snap = s.snapshot()
        oa = hb.brakingbase_open(a, x); after_a = [libc.random() for _ in range(4)]
        s.restore(snap)
        ob = hb.brakingbase_open_any(b, x); after_b = [libc.random() for _ in range(4)]
        s.restore(snap)
        oc = hb.brakingbase_open_any(a, x)                      # a commitment of the existing commit is served too
    finally:
        s.close()
    same(ob, oa, "open_any"); same(oc, oa, "open_any of commit's object")
    assert after_a == after_b
    check_opening(ob, K, "(2^%d, %d)" % (logn, K))
    a.free(); b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 4])
def test_encode_at_2e21(hb, oracle, code21, rows21, rows):
    """every entry of every codeword, the zero tail too, against encode_monolithic"""
    src = np.ascontiguousarray(rows21["poly"].reshape(4, N21, 2)[:rows].transpose(1, 0, 2))
    got = hb.encode_interleaved(src)
    assert got.shape == (2 * N21, rows, 2)
    for i in range(rows):
        assert np.array_equal(got[:, i], rows21["T"][i]), i
    assert not got[code21["len"]:].any()


@pytest.mark.gpu
def test_code_proof_at_2e21(hb, oracle, code21, rows21):
    oracle_graphs(oracle, N21)
    r1 = pyoracle.splitmix_field(22, 99)
    got = hb.prove_linear_code(rows21["T"][0], N21, r1)
    want = oracle.prove_linear_code(rows21["T"][0], N21, r1)
    same(got, want, "prove_linear_code")
    assert claim(got["poly"][0]) == ZERO


@pytest.mark.gpu
@pytest.mark.parametrize("quirk", [1, 0])
def test_commit_any_at_2e23_4(hb, code21, rows21, quirk):
    """the root against the tree of tests/commit_refs.py over the column digests of the oracle's codewords"""
    c = hb.brakingbase_commit_any(rows21["poly"], 4, quirk=quirk)
    assert (c.N, c.K, c.trs, c.len) == (1 << 23, 4, N21, code21["len"])
    dig = commit_refs.col_digests(rows21["T"], 4, quirk)
    assert np.array_equal(c.root(), commit_refs.tree(dig, quirk)[-1])
    assert np.array_equal(c.tensor(N21 - 1, 3), rows21["T"][:, N21 - 1:N21 + 2])
    with pytest.raises(_mod().HobbitError, match="rc=-2"):
        hb.brakingbase_open(c, pyoracle.splitmix_field(2, 5))   # the existing opening keeps its cap
    c.free()
    h = ctypes.c_void_p()
    d = hb.alloc(16)
    rc = hb.lib.hobbit_brakingbase_commit_any(hb.ctx, ctypes.c_void_p(d.ptr), ctypes.c_size_t(1 << 24), ctypes.c_size_t(4), ctypes.c_int(1), ctypes.byref(h))
    assert rc == -2 and not h.value and b"2^31" in hb.lib.hobbit_last_error(hb.ctx)


@pytest.fixture(scope="module")
def lists21(hb, code21):
    """the device-built commitment of 2^21: its shape, lists and root; freed before anything else is built"""
    m, Pn = hb.parity_shape(N21)
    a = hb.commit_parity_matrix_device(N21)
    out = dict(m=m, P=Pn, dims=(a.n, a.m, a.P), lists=a.lists(), root=a.root())
    a.free()
    return out


@pytest.mark.gpu
def test_lists_at_2e21_host_and_device_builders_agree(hb, code21, lists21):
    assert lists21["P"] == 1 << 26 and 1 << 25 < lists21["m"] <= 1 << 26 and lists21["dims"] == (N21, lists21["m"], 1 << 26)
    b = hb.commit_parity_matrix(N21)
    assert (b.n, b.m, b.P) == lists21["dims"]
    want = b.lists()
    assert np.array_equal(b.root(), lists21["root"])
    b.free()
    for k in ("idx1", "idx2", "cnt1", "cnt2", "weight", "acc1", "acc2"):
        assert np.array_equal(lists21["lists"][k], want[k]), k


@pytest.fixture(scope="module")
def open21(hb, oracle, code21, rows21):
    """one hobbit_brakingbase_open_any at (2^23, 4), the libc stream it started from, and the aggregate of C_p rebuilt from a fresh commitment"""
    c = hb.brakingbase_commit_any(rows21["poly"], 4)
    x = pyoracle.splitmix_field(2, 5)
    s = LibcStream(2121)
    try:
        snap = s.snapshot()
        t0 = time.perf_counter()
        o = hb.brakingbase_open_any(c, x)
        print("hobbit_brakingbase_open_any(2^23, 4): %.2f s, stages (ms) %s" % (time.perf_counter() - t0, np.round(o["stage_ms"], 1).tolist()))
    finally:
        s.close()
    c.free()
    return dict(o=o, snap=snap)


def whir_direct(hb, d_aggr, w, x, snap, skip):
    """hobbit_whir_commit + hobbit_whir_prove_any on the device buffer d_aggr (w F) at x, the libc stream `skip` draws after the snapshot"""
    com, lv = hb.alloc(32 * w), hb.alloc(32 * w)
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d_aggr, w, com.ptr, lv.ptr))
    s = LibcStream(1)
    try:
        s.restore(snap, skip=skip)
        res = hb.whir_prove_any((d_aggr, w), x, com, lv)
    finally:
        s.close()
    res["whir_root"] = hb.to_host(lv, (32,), np.uint8, offset=32 * (w - 2))
    return res


def same_whir(sp, res, what):
    for a, b in (("wq", "poly"), ("wa", "a"), ("wroots", "roots"), ("wscal", "scal"), ("wchecks", "checks"), ("iters", "iters"), ("whir_root", "whir_root"),
                 ("qn", "qn"), ("qidx", "qidx"), ("qreply", "qreply"), ("qpaths", "qpaths"), ("final_pb", "final_pb")):
        assert np.array_equal(np.asarray(sp[a]).reshape(-1), np.asarray(res[b]).reshape(-1)), what + "/" + a


@pytest.mark.gpu
def test_open_any_at_2e23_4_round_tests(open21):
    """checks == [1, 1], P1's claimed sum is zero, and every sumcheck passes the verifier's round test: P1 .. P4, both trees, P1 / P2 of sp_p,
    sp_w and sp_c, and the WHIR checks"""
    o = open21["o"]
    check_opening(o, 4, "(2^23, 4)")
    assert int(o["parity"]["sp_p"]["iters"][0]) >= 1 and int(o["parity"]["sp_w"]["iters"][0]) >= 1 and int(o["sp_c"]["iters"][0]) >= 1
    assert len(o["parity"]["p2"]["poly"]) == 26 and len(o["parity"]["p4"]["poly"]) == 29


@pytest.mark.gpu
def test_open_any_at_2e23_4_p2_claim_without_the_lists(hb, oracle, code21, open21):
    """P2's claimed sum is eq(r2)^T A(r1): A from hobbit_parity_matrix and from the oracle's evaluate_parity_matrix, neither of which reads the lists"""
    o = open21["o"]
    r1, r2 = o["p1"]["r"], o["p1"]["r1"]                     # open_parity_matrix(P1.randomness[0], P1.randomness[1])
    oracle_graphs(oracle, N21)
    A = hb.evaluate_parity_matrix(hb.precompute_beta(r1), N21)
    A_orc, ln = oracle.evaluate_parity_matrix(oracle.precompute_beta(r1), N21)
    assert ln == code21["len"] and np.array_equal(A, A_orc)
    want = fi(hb.evaluate_vector(A, r2))
    assert want == fi(oracle.evaluate_vector(A_orc, r2))
    assert claim(o["parity"]["p2"]["poly"][0]) == want


@pytest.mark.gpu
def test_open_any_at_2e23_4_nested_whir_of_sp_p(hb, oracle, code21, lists21, open21):
    """C_p's root is the device-built commitment's, and the nested WHIR proof of shockwave_prove(C_p) -- width 2^25, the table-free
    out-of-domain step -- is hobbit_whir_commit + hobbit_whir_prove_any of the same aggregate at sp_p.r2, from the same place of the libc stream
    (found on the stream by the proof's own first four fold challenges)"""
    o = open21["o"]; sp = o["parity"]["sp_p"]
    assert np.array_equal(o["cp_root"], lists21["root"])
    Pn = lists21["P"]; w = 8 * Pn // 16
    assert w == 1 << 25 and int(sp["iters"][0]) >= 1
    pc = hb.commit_parity_matrix_device(N21)
    assert np.array_equal(pc.root(), o["cp_root"])
    beta = oracle.precompute_beta(o["parity"]["p4"]["r"][-4:])            # beta1 of shockwave_prove: the last log2 16 coordinates
    aggr = hb.alloc(16 * w)
    hb._chk(hb.lib.hobbit_aggregate(hb.ctx, ctypes.c_void_p(pc.dev(7)), ctypes.c_size_t(8 * Pn), beta.ctypes.data_as(ctypes.c_void_p), 16, ctypes.c_void_p(aggr.ptr)))
    hb.sync()
    pc.free()
    s = LibcStream(1)
    try:
        skip = s.find(open21["snap"], [int(v) for v in sp["wa"][:4, 0]])
    finally:
        s.close()
    res = whir_direct(hb, aggr.ptr, w, sp["r2"], open21["snap"], skip)
    assert res["checks"].tolist() == [1, 1]
    same_whir(sp, res, "sp_p")


@pytest.mark.gpu
def test_shockwave_prove_alone_at_width_2e25(hb):
    """hobbit_shockwave_prove at k = 1, N = 2^25 (the routing to the table-free step without the parity code around it) against the direct call"""
    N = 1 << 25
    d = hb.fill_splitmix(N, 3)
    enc = hb.alloc(32 * N)
    hb._chk(hb.lib.hobbit_fill_splitmix(hb.ctx, ctypes.c_void_p(enc.ptr), ctypes.c_size_t(N), ctypes.c_uint64(3)))
    hb._chk(hb.lib.hobbit_memset(hb.ctx, ctypes.c_void_p(enc.ptr + 16 * N), 0, ctypes.c_size_t(16 * N)))
    hb._chk(hb.lib.hobbit_fft_any(hb.ctx, ctypes.c_void_p(enc.ptr), 26, 1, 2 * N, 0))
    out, o = hb._sp_buffers(N, 1)
    x = np.zeros((1, 2), np.uint64)
    s = LibcStream(77)
    try:
        snap = s.snapshot()
        hb._chk(hb.lib.hobbit_shockwave_prove(hb.ctx, d.ptr, enc.ptr, None, N, 1, x.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(o)))
    finally:
        s.close()
    sp = hb._sp_trim(out, N, 1)
    assert int(sp["iters"][0]) >= 1
    check_shockwave(sp, "k = 1")
    res = whir_direct(hb, d.ptr, N, sp["r2"], snap, 240)       # the 240 query columns come first (src/Virgo.cpp:463-467)
    assert res["checks"].tolist() == [1, 1]
    same_whir(sp, res, "k = 1")
