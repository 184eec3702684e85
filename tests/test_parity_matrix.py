"""The code's parity matrix, committed and opened (include/hobbit_parity.h): commit_parity_matrix, open_parity_matrix, prove_linear_code_batch
(src/sumcheck.cpp:2622-2885, 3201-3221).

Three layers of evidence:
  * tests/golden/parity_matrix.npz -- the REAL reference (scripts/gen_parity_golden.py), as far as it can run: C_p, the lists, C_w's root and the
    mimc transcript up to its first SHA3 call (inside the first _whir_prove of shockwave_prove(C_p)), under a zero-filling allocator; the
    whole batch proofs;
  * tests/parity_model.py -- both functions restated from the oracle's primitives with index padding 0; pinned here, on the CPU, by the fixture
    record for record, and covering everything behind the first SHA3 call;
  * the device (-m gpu): every output against the model, the library's own transcript recorder against the fixture.
Every input lies on the libc stream of a fresh process (srandom(1); expander_init_store(n) first), as the fixture's runs do.
"""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import parity_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "parity_matrix.npz")
NS = (128, 1024, 4096)
BATCHES = ((128, 2), (128, 64), (4096, 4))
libc = ctypes.CDLL(None)
libc.random.restype = ctypes.c_long


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def _mod():
    from __graft_entry__ import load_package
    return load_package()


def graphs(orc, n):
    levels, dep, m = {}, 0, n
    while m > 13:
        for kind in (0, 1):
            levels[(dep, kind)] = orc.graph(dep, kind)
        m = int(0.211 * m); dep += 1
    return levels


def start(orc, n):
    """the libc stream of a fresh process up to the call of open_parity_matrix: the graphs of n, then r1 and r2"""
    orc.rng_reset()
    orc.expander_init_store(n)
    l = (2 * n).bit_length() - 1
    return orc.generate_randomness(l), orc.generate_randomness(l)


_MODEL = {}


def model(orc, n, opened=True):
    """commit (and opening) of the model at n on the fresh-process stream, computed once"""
    if (n, False) not in _MODEL:
        start(orc, n)
        _MODEL[(n, False)] = dict(C=pm.commit(orc, n))
    if opened and (n, True) not in _MODEL:
        res, rec = model_transcript(orc, n)
        _MODEL[(n, True)] = dict(C=_MODEL[(n, False)]["C"], open=res, records=rec)
    return _MODEL[(n, opened)]


# ---- the transcript a proof implies: every record (x, k, mimc(x, k)) in the reference's order -------------------------------------------------
class Transcript:
    def __init__(self, orc):
        self.orc, self.rec = orc, []

    def h(self, x, k):
        o = self.orc.mimc(np.asarray(x, np.uint64).reshape(1, 2), np.asarray(k, np.uint64).reshape(1, 2))[0]
        self.rec.append(np.concatenate([np.asarray(x, np.uint64).reshape(2), np.asarray(k, np.uint64).reshape(2), o]))
        return o

    def sumcheck(self, seed, poly, r, vr, fin, cubic):
        """generate_2product_sumcheck_proof (:2422-2446) / _generate_3product_sumcheck_proof (:2016-2045: the challenge of a round is the state
        BEFORE its polynomial is hashed)"""
        rand = np.asarray(seed, np.uint64).reshape(2)
        for i in range(poly.shape[0]):
            if cubic and r is not None and i < len(r):
                assert np.array_equal(r[i], rand)
            for c in poly[i]:
                rand = self.h(rand, c)
            if not cubic and r is not None and i < len(r):
                assert np.array_equal(r[i], rand)
        rand = self.h(rand, vr[0]); rand = self.h(rand, vr[1])
        assert np.array_equal(np.asarray(fin).reshape(2), rand)
        return rand

    def tree(self, t, x_last):
        """prove_multiplication_tree_new with more than one vector and no prev_x (:172-209)"""
        prev = self.h(x_last, t["out_eval"])
        off = 0
        for k in range(int(t["layers"][0])):
            rounds = 2 + k
            prev = self.sumcheck(prev, t["poly"][off:off + rounds], t["r"][off:off + rounds], t["vr"][k], t["fin"][k], True)
            off += rounds

    def shockwave_head(self, sp):
        """shockwave_prove up to _whir_prove: P1 seeded with F(33), prove_fft seeded with P1's last challenge (src/Virgo.cpp:476-477)"""
        self.sumcheck(pm.Fi(33), sp["q1"], sp["r1"], sp["vr1"], sp["fin1"], False)
        self.sumcheck(sp["r1"][-1], sp["q2"], sp["r2"], sp["vr2"], sp["fin2"], False)

    def records(self):
        return np.stack(self.rec)


def peek_randomness(orc, k):
    """generate_randomness(k) as the NEXT caller will see it, without consuming it: when another state array is switched in, glibc writes the
    generator's position into the first word of the one it leaves (the pointer initstate returns), so a byte copy of that array (128 bytes:
    the default TYPE_3 state) replays it"""
    libc.initstate.restype = ctypes.c_void_p; libc.initstate.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
    libc.setstate.restype = ctypes.c_void_p; libc.setstate.argtypes = [ctypes.c_void_p]
    tmp = ctypes.create_string_buffer(256)
    cur = libc.initstate(1, tmp, 256)
    clone = ctypes.create_string_buffer(ctypes.string_at(cur, 128), 256)
    libc.setstate(ctypes.addressof(clone))
    r = orc.generate_randomness(k)
    libc.setstate(cur)
    return r


def model_transcript(orc, n):
    """the model's opening at n again, this time noting the two generate_randomness(2) of the trees, turned into the record sequence"""
    C = model(orc, n, opened=False)["C"]
    r1, r2 = start(orc, n)
    seen = []
    real = orc.mul_tree

    def spy(inp, previous_r, prev_x=None):
        seen.append(peek_randomness(orc, 2))
        return real(inp, previous_r, prev_x)
    orc.mul_tree = spy
    try:
        res = pm.open_(orc, C, r1, r2)
    finally:
        del orc.mul_tree
    T = Transcript(orc)
    T.tree(res["t1"], seen[0][-1]); T.tree(res["t2"], seen[1][-1])
    T.sumcheck(pm.Fi(321), res["p2"]["poly"], res["p2"]["r"], res["p2"]["vr"], res["p2"]["fin"], True)
    T.sumcheck(pm.Fi(321), res["p3"]["poly"], res["p3"]["r"], res["p3"]["vr"], res["p3"]["fin"], False)
    T.sumcheck(pm.Fi(321), res["p4"]["poly"], res["p4"]["r"], res["p4"]["vr"], res["p4"]["fin"], False)
    T.shockwave_head(res["sp_p"])
    return res, T.records()


# ---- CPU: model against the real reference's fixture -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_model_commit_matches_reference(oracle, gold, n):
    C = model(oracle, n, opened=False)["C"]
    k = "_%d" % n
    assert C["m"] == int(gold["m" + k][0]) and C["P"] == int(gold["P" + k][0])
    m = C["m"]
    assert np.array_equal(dg(C["idx1"][:m].astype(np.uint32)), gold["idx1_dg" + k]) and np.array_equal(dg(C["idx2"][:m].astype(np.uint32)), gold["idx2_dg" + k])
    assert np.array_equal(dg(C["weight"][:m]), gold["weight_dg" + k])
    assert np.array_equal(C["root"], gold["cp_root" + k])
    off, sz, lv = 0, C["P"], 0
    while sz >= 1:
        assert np.array_equal(dg(C["levels"][off:off + sz]), gold["cp_level_dg" + k][lv]), "C_p level %d" % lv
        off += sz; sz //= 2; lv += 1
    assert lv == gold["cp_level_dg" + k].shape[0]


@pytest.mark.parametrize("n", NS)
def test_model_transcript_matches_reference(oracle, gold, n):
    """record for record up to the reference's first SHA3 call: both trees, P2, P3, P4 and the two sumchecks of shockwave_prove(C_p)"""
    k = "_%d" % n
    r1, r2 = start(oracle, n)
    assert np.array_equal(r1, gold["r1" + k]) and np.array_equal(r2, gold["r2" + k])
    M = model(oracle, n)
    res, rec, want = M["open"], M["records"], gold["transcript" + k]
    assert rec.shape == want.shape, (rec.shape, want.shape)
    bad = np.nonzero((rec != want).any(axis=1))[0]
    assert not len(bad), "first differing record: %d" % bad[0]
    assert np.array_equal(res["cw_root"], gold["cw_root" + k])
    assert res["checks"].tolist() == [1, 1]


def test_fixture_records_the_allocator_dependence(gold):
    """the reference's transcript is not a function of its inputs (reads past access_idx's size): another fill byte changed it, C_p not"""
    assert int(gold["malloc_perturb"][0]) == 255 and int(gold["other_perturb"][0]) != 255
    assert int(gold["other_first_diff"][0]) >= 0 and int(gold["other_cp_root_equal"][0]) == 1


def batch_inputs(orc, n, count):
    """the fixture's inputs: graphs of n first, then `count` codewords = encode_monolithic(generate_randomness(n)) (2n F each), then r1, r2"""
    orc.rng_reset(); orc.expander_init_store(n)
    cw = np.stack([orc.encode_monolithic(orc.generate_randomness(n))[0] for _ in range(count)])
    return cw, orc.generate_randomness((2 * n).bit_length() - 1), orc.generate_randomness(count.bit_length() - 1)


@pytest.mark.parametrize("n,count", BATCHES)
def test_model_batch_matches_reference(oracle, gold, n, count):
    k = "batch_%d_%d_" % (n, count)
    cw, r1, r2 = batch_inputs(oracle, n, count)
    assert np.array_equal(dg(cw), gold[k + "cw_dg"]) and np.array_equal(r1, gold[k + "r1"]) and np.array_equal(r2, gold[k + "r2"])
    got = pm.prove_linear_code_batch(oracle, cw, n, r1, r2)
    for f in ("poly", "r", "vr", "fin"):
        assert np.array_equal(got[f], gold[k + f]), f
    assert np.array_equal(oracle.claim_of(got["poly"][0]), np.zeros(2, np.uint64)), "genuine codewords: the claimed sum is zero"


# ---- the header and its symbols (CPU) -------------------------------------------------------------------------------------------------------------
ASYNC = {"hobbit_parity_commit"}
HOST_RETURNING = {"hobbit_parity_open", "hobbit_prove_linear_code_batch", "hobbit_parity_root", "hobbit_parity_levels", "hobbit_parity_lists"}
EXEMPT = {
    "hobbit_parity_commitment_free": "free function: waits for the stream",
    "hobbit_parity_dims": "accessor, host only",
    "hobbit_parity_dev": "accessor of raw device pointers",
}


def declared():
    src = open(os.path.join(ROOT, "include", "hobbit_parity.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    from __graft_entry__ import build_hip
    build_hip()
    mod = _mod()
    lib = mod.load_library()
    decl = declared()
    assert len(decl) == 9 and sorted(mod.PARITY_SYMBOLS) == decl
    for s in decl:
        assert hasattr(lib, s), "missing export " + s
        assert getattr(lib, s).argtypes is not None, "no prototype bound for " + s
    assert not set(decl) & set(mod.ABI_SYMBOLS)
    for meth in ("commit_parity_matrix", "open_parity_matrix", "prove_linear_code_batch"):
        assert callable(getattr(mod.Hobbit, meth))


def test_every_export_is_classified():
    """what tests/test_async_contract.py asks of hobbit_hip.h, for the second header: asynchronous (with a stream test below), host-returning or exempt"""
    sets = {"ASYNC": ASYNC, "HOST_RETURNING": HOST_RETURNING, "EXEMPT": set(EXEMPT)}
    names = set(declared())
    for n in sorted(names):
        assert len([k for k, s in sets.items() if n in s]) == 1, n
    for k, s in sets.items():
        assert not (s - names), (k, sorted(s - names))


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)
    yield h
    h.close()


def same(a, b, what):
    if isinstance(b, dict):
        for k in b:
            same(a[k], b[k], what + "/" + k)
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def same_opening(got, want):
    for k in ("t1", "t2", "p2", "p3", "p4", "cw_root", "scalars", "partial", "acc_y", "checks", "sp_p", "sp_w"):
        same(got[k], want[k], k)


def check_commit(pc, C):
    assert (pc.n, pc.m, pc.P) == (C["n"], C["m"], C["P"])
    ls = pc.lists()
    for k in ("idx1", "idx2", "cnt1", "cnt2"):
        assert np.array_equal(ls[k].astype(np.int64), C[k]), k
    for k in ("weight", "acc1", "acc2"):
        assert np.array_equal(ls[k], C[k]), k
    assert np.array_equal(pc.levels(), C["levels"]) and np.array_equal(pc.root(), C["root"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 128, 1024, 4096, 8192])
def test_commit_on_the_device(hb, oracle, gold, n):
    """lists, levels and root against the model at every size (16: commit only; 8192: the long-code graphs), against the fixture where it has the size"""
    C = model(oracle, n, opened=False)["C"]
    start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    pc = hb.commit_parity_matrix(n)
    check_commit(pc, C)
    if n in NS:
        k = "_%d" % n
        assert pc.m == int(gold["m" + k][0]) and pc.P == int(gold["P" + k][0]) and np.array_equal(pc.root(), gold["cp_root" + k])
        ls = pc.lists()
        assert np.array_equal(dg(ls["idx1"][:pc.m]), gold["idx1_dg" + k]) and np.array_equal(dg(ls["idx2"][:pc.m]), gold["idx2_dg" + k])
        assert np.array_equal(dg(ls["weight"][:pc.m]), gold["weight_dg" + k])
        lv, off, sz = pc.levels(), 0, pc.P
        for d in gold["cp_level_dg" + k]:
            assert np.array_equal(dg(lv[off:off + sz]), d)
            off += sz; sz //= 2
    pc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 1024, 4096, 8192])
def test_open_on_the_device(hb, oracle, gold, n):
    """every output against the model, both checks hold, and the library's own transcript equals the real reference's over the fixture's length"""
    want = model(oracle, n)
    r1, r2 = start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    pc = hb.commit_parity_matrix(n)
    hb.lib.hobbit_transcript_record(1)
    try:
        got = hb.open_parity_matrix(pc, r1, r2)
        cnt = hb.lib.hobbit_transcript_count()
        rec = np.zeros((cnt, 6), np.uint64)
        hb.lib.hobbit_transcript_read(rec.ctypes.data_as(ctypes.c_void_p), cnt)
    finally:
        hb.lib.hobbit_transcript_record(0)
    assert got["checks"].tolist() == [1, 1]
    same_opening(got, want["open"])
    if n in NS:
        ref = gold["transcript_%d" % n]
        assert cnt > ref.shape[0]
        bad = np.nonzero((rec[:ref.shape[0]] != ref).any(axis=1))[0]
        assert not len(bad), "first differing record: %d" % bad[0]
        assert np.array_equal(got["cw_root"], gold["cw_root_%d" % n])
    pc.free()


def next_draws(seed, k=4):
    libc.srandom(seed)
    return [libc.random() for _ in range(k)]


@pytest.mark.gpu
def test_refusals(hb, oracle):
    mod = _mod()
    r1, r2 = start(oracle, 64); hb.upload_graphs(64, graphs(oracle, 64))
    pc = hb.commit_parity_matrix(64)                     # P = 1024: committed, but below the nested WHIR proofs' smallest width
    assert pc.P == 1024
    want = next_draws(5)
    libc.srandom(5)
    with pytest.raises(mod.HobbitError, match="rc=-2"):
        hb.open_parity_matrix(pc, r1, r2)
    assert [libc.random() for _ in range(4)] == want, "a refused opening drew from libc"
    pc.free()
    with pytest.raises(mod.HobbitError, match="rc=-2"):
        hb.commit_parity_matrix(100)
    r1, r2 = start(oracle, 128); hb.upload_graphs(128, graphs(oracle, 128))
    with pytest.raises(mod.HobbitError, match="rc=-5"):
        hb.commit_parity_matrix(256)                     # graphs finalized for another n
    pc = hb.commit_parity_matrix(128)
    libc.srandom(5)
    for bad in (np.concatenate([r1, r1[:1]]), r1[:-1]):
        with pytest.raises(mod.HobbitError, match="rc=-2"):
            hb.open_parity_matrix(pc, bad, bad)
    assert [libc.random() for _ in range(4)] == want
    pc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", BATCHES + ((4096, 64),))
def test_batch_on_the_device(hb, oracle, gold, n, count):
    cw, r1, r2 = batch_inputs(oracle, n, count)
    hb.upload_graphs(n, graphs(oracle, n))
    want = pm.prove_linear_code_batch(oracle, cw, n, r1, r2)
    got = hb.prove_linear_code_batch(cw, n, r1, r2)
    same(got, want, "batch")
    if (n, count) in BATCHES:
        for f in ("poly", "r", "vr", "fin"):
            assert np.array_equal(got[f], gold["batch_%d_%d_%s" % (n, count, f)]), f
    # codewords shorter than 2n: the reference's B is zero past their end
    ln = 2 * n - 3
    same(hb.prove_linear_code_batch(np.ascontiguousarray(cw[:, :ln]), n, r1, r2), pm.prove_linear_code_batch(oracle, cw[:, :ln], n, r1, r2), "short codewords")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 4096])
def test_mirror_hook(hb, oracle, n):
    """commit_parity_matrix / open_parity_matrix of the C++ mirror (its own context, its own draws from srandom(1)): the bits of the C ABI run on the
    same stream, and ps equal to the model's sum"""
    from __graft_entry__ import PKG, build_host
    build_host()
    want = model(oracle, n)
    r1, r2 = start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    pc = hb.commit_parity_matrix(n); abi = hb.open_parity_matrix(pc, r1, r2); root = pc.root(); P = pc.P; pc.free()
    L = P.bit_length() - 1
    lib = ctypes.CDLL(os.path.join(PKG, "libhobbit_host.so"))
    roots = np.zeros((4, 32), np.uint8); polys = np.zeros((4 * L + 3 * (L + 1) + 3 * (L + 3), 2), np.uint64); scal = np.zeros((13, 2), np.uint64)
    checks = np.zeros(4, np.int32); ps = ctypes.c_double(0)
    V = ctypes.c_void_p
    lib.hobbit_host_parity_open.argtypes = [ctypes.c_int, ctypes.c_uint] + [V] * 5
    rounds = lib.hobbit_host_parity_open(n, 0, *[a.ctypes.data_as(V) for a in (roots, polys, scal, checks)], ctypes.byref(ps))
    lib.hobbit_host_close()
    assert rounds == L + 3 and checks.tolist() == [1, 1, 1, 1]
    assert np.array_equal(roots[0], root) and np.array_equal(roots[1], abi["cw_root"])
    assert np.array_equal(roots[2], abi["sp_p"]["whir_root"]) and np.array_equal(roots[3], abi["sp_w"]["whir_root"])
    assert np.array_equal(polys, np.concatenate([abi[p]["poly"].reshape(-1, 2) for p in ("p2", "p3", "p4")]))
    assert np.array_equal(scal, np.concatenate([abi["scalars"], abi["partial"], abi["acc_y"]]))
    assert ps.value == pm.open_proof_size(want["open"], P), (ps.value, pm.open_proof_size(want["open"], P))


# ---- the stream contract: hobbit_parity_commit is asynchronous -----------------------------------------------------------------------------------------
BACKLOG_REPS, BACKLOG_N = 1000, 1 << 24      # the backlog of tests/test_async_contract.py: about 160 ms of element-wise products on the device


@pytest.mark.gpu
def test_commit_queued_behind_a_backlog_then_opened(hb, oracle):
    """commit on a caller's (torch) stream behind a backlog, the opening right behind it with no synchronisation in between: the bits of the
    synchronised run on the library's own stream"""
    import torch
    n = 128
    r1, r2 = start(oracle, n); levels = graphs(oracle, n)
    hb.upload_graphs(n, levels)
    pc = hb.commit_parity_matrix(n); hb.sync()
    libc.srandom(77); want = hb.open_parity_matrix(pc, r1, r2); root = pc.root(); pc.free()
    stream = torch.cuda.Stream()
    hs = _mod().Hobbit(0, stream=stream.cuda_stream)
    try:
        hs.upload_graphs(n, levels)
        w = hs.commit_parity_matrix(n); libc.srandom(3); hs.open_parity_matrix(w, r1, r2); w.free()      # the shapes once: workspaces grow now
        t = [torch.empty((BACKLOG_N, 2), dtype=torch.int64, device="cuda") for _ in range(3)]
        for i in range(2):
            hs._chk(hs.lib.hobbit_fill_splitmix(hs.ctx, t[i].data_ptr(), BACKLOG_N, 77 + i))
        hs.sync()
        for _ in range(BACKLOG_REPS):
            hs._chk(hs.lib.hobbit_f_binop(hs.ctx, 2, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), BACKLOG_N))
        pc2 = hs.commit_parity_matrix(n)
        busy = not stream.query()
        libc.srandom(77); got = hs.open_parity_matrix(pc2, r1, r2)
        assert np.array_equal(pc2.root(), root)
        same_opening(got, want)
        assert busy, "the commit returned to an idle stream: it waited, or the backlog is too short"
        pc2.free()
    finally:
        hs.close()
