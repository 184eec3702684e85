"""tests/open_verifier.py held by the oracle, without a GPU: the verifier accepts the oracle's openings and shockwave proofs, rejects a one-bit
change of whatever it reads (the entries it cannot see are listed by rule, not found by running it), and rejects an opening made with another
polynomial than the committed one -- which the prover's own `checks` do not notice."""
import ctypes

import numpy as np
import pytest

import open_verifier as ov
from open_verifier import Rejected, fi
from oracle import pyoracle

libc = ctypes.CDLL(None)
_CACHE = {}


def oracle_ends(orc, poly, x, K, trs):
    """the aggregate, the parity half C of its tensor code, and ends(pc, pa) over them (the graphs of trs are the oracle's current ones)"""
    logK = K.bit_length() - 1
    aggr = orc.aggregate(poly, orc.precompute_beta(x[:logK]))
    cols = 2 * len(aggr) // trs
    C = np.ascontiguousarray(orc.compute_tensorcode(aggr, trs, 1).reshape(2 * trs, cols, 2)[trs:].reshape(-1, 2))
    seen = {}

    def ends(pc, pa):
        key = pc.tobytes() + pa.tobytes()
        if key not in seen:
            seen[key] = (fi(orc.evaluate_vector(C, pc)), fi(orc.evaluate_vector(aggr, pa)))
        return seen[key]
    return aggr, C, ends


def opening(orc, logN, K, queries, seed=777, other=False):
    """the oracle's commit and opening of splitmix_field(N, 5) at a drawn point; other: opened with a polynomial that differs from the committed
    one in one bit of one coefficient, the tensor being the committed one's"""
    key = (logN, K, queries, seed, other)
    if key not in _CACHE:
        N = 1 << logN; trs = N // (K << 11)
        orc.rng_reset(); orc.expander_init_store(trs)
        poly = pyoracle.splitmix_field(N, 5); x = pyoracle.splitmix_field(logN, 6)
        _, T = orc.commit_standard(poly, K, trs, 1, want_tensor=True)
        if other:
            poly = poly.copy(); poly[N // 3, 0] ^= np.uint64(1)
        libc.srandom(seed); o = orc.open_standard(poly, K, trs, x, queries, tensor=T)
        aggr, C, ends = oracle_ends(orc, poly, x, K, trs)
        _CACHE[key] = dict(o=o, x=x, K=K, trs=trs, ends=ends, aggr=aggr, C=C)
    return _CACHE[key]


def verify_all(orc, c):
    """verify_open and verify_shockwave of sp_c and sp_f"""
    o, x, K, trs = c["o"], c["x"], c["K"], c["trs"]
    cl = ov.verify_open(o, x, K, trs, c["ends"])
    pc, _, pf = ov.open_points(o, x, K, trs)
    ov.verify_shockwave(o["sp_c"], pc, 32, ov.matrix_end(lambda p: orc.evaluate_vector(c["C"], p), pc, 32), "sp_c")
    ov.verify_shockwave(o["sp_f"], pf, 32, ov.matrix_end(lambda p: orc.evaluate_vector(c["aggr"], p), pf, 32), "sp_f")
    return cl


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------------------
def test_eq_at_is_precompute_beta(oracle):
    r = pyoracle.splitmix_field(5, 3); b = oracle.precompute_beta(r)
    assert all(fi(b[i]) == ov.eq_at(r, i) for i in range(32))
    u = pyoracle.splitmix_field(5, 4)
    assert ov.eq_points(u, r) == fi(oracle.evaluate_vector(b, u))
    s = fi(pyoracle.splitmix_field(1, 9)[0]); pw, tab = ov.ONE, []
    for _ in range(32):
        pw = ov.fmul(pw, s); tab.append(pw)
    assert ov.powers_mle(s, r) == fi(oracle.evaluate_vector(np.array(tab, np.uint64), r))


@pytest.mark.parametrize("logN,K,queries", [(16, 4, 1), (16, 4, 2), (16, 4, 300), (18, 32, 5900), (20, 32, 5900)])
def test_the_oracles_opening_is_accepted(oracle, logN, K, queries):
    """(2^18, 32): trs = 4, the identity code; sp_f has width 256 and no WHIR proof, sp_c width 512 and one"""
    c = opening(oracle, logN, K, queries)
    o = c["o"]
    assert o["checks"].tolist() == [1, 1, 1]
    cl = verify_all(oracle, c)
    assert cl[0] == ov.ZERO and len(cl) == 5
    if (logN, K) == (18, 32):
        assert c["trs"] == 4 and int(o["sp_f"]["iters"][0]) == 0 and int(o["sp_c"]["iters"][0]) >= 1
        assert len(o["sp_f"]["q1"]) == 9 and len(o["sp_c"]["q1"]) == 10      # rounds over the doubled widths 512 and 1024
    if queries == 5900:
        assert len(ov.last_writes(o["I"], 4096)) < queries       # overwritten positions are there to be handled


def shockwave(orc, logN, k):
    key = ("sp", logN, k)
    if key not in _CACHE:
        N = 1 << logN
        m = pyoracle.splitmix_field(N, 3); x = pyoracle.splitmix_field(logN, 4)
        enc, lv = orc.shockwave_commit(m, k)
        libc.srandom(5); sp = orc.shockwave_prove(m, enc, k, x, lv)
        _CACHE[key] = dict(sp=sp, x=x, k=k, m=m, end=ov.matrix_end(lambda p: orc.evaluate_vector(m, p), x, k))
    return _CACHE[key]


@pytest.mark.parametrize("logN,k", [(10, 4), (12, 8), (14, 32), (15, 32)])
def test_the_oracles_shockwave_proof_is_accepted(oracle, logN, k):
    c = shockwave(oracle, logN, k)
    ov.verify_shockwave(c["sp"], c["x"], k, c["end"])
    assert (int(c["sp"]["iters"][0]) > 0) == ((1 << logN) // k > 256)
    # the end is the row's evaluation: row = sum_j eq(x[-log2 k:])[j] matrix[j], built here entry by entry
    lk = k.bit_length() - 1; w = (1 << logN) // k
    beta = oracle.precompute_beta(c["x"][logN - lk:])
    row = np.zeros((w, 2), np.uint64)
    for j in range(k):
        row = oracle.f_add(row, oracle.f_mul(np.tile(beta[j], (w, 1)), np.ascontiguousarray(c["m"].reshape(k, w, 2)[j])))
    r2 = np.ascontiguousarray(c["sp"]["r2"])
    assert c["end"](r2) == fi(oracle.evaluate_vector(row, r2))


# ---- one-bit changes ----------------------------------------------------------------------------------------------------------------------------------
def accepted_after_flips(arr, idxs, verify):
    """the flat indices of arr whose lowest bit can be changed without verify() raising Rejected"""
    flat = arr.reshape(-1)
    assert np.shares_memory(flat, arr)
    acc = []
    for i in idxs:
        old = flat[i].copy(); flat[i] = old ^ type(old)(1)
        try:
            verify(); acc.append(int(i))
        except Rejected:
            pass
        flat[i] = old
    return acc


def sample(size, n, seed):
    return range(size) if size <= n else sorted(np.random.default_rng(seed).choice(size, n, replace=False).tolist())


def overwritten(positions):
    """the queries whose position a later query has too"""
    last = {p: q for q, p in enumerate(positions)}
    return {q for q, p in enumerate(positions) if last[p] != q}


def moves_unseen(positions, q, new):
    """moving query q to `new` leaves the last-write-wins map as it is: q was overwritten where it stood, and is overwritten where it goes"""
    return any(p == positions[q] for p in positions[q + 1:]) and any(p == new for p in positions[q + 1:])


@pytest.mark.parametrize("key", ["poly", "r", "vr", "scalars", "reply", "I"])
def test_one_bit_changes_of_the_opening_are_rejected(oracle, key):
    """(2^16, 4), 300 queries, libc seed 777.  Every entry of poly, r, vr and scalars, 600 seeded entries each of reply and I.  Accepted are exactly
      * scalars[0] (rv0 feeds nothing the verifier reads),
      * the replies of queries whose position a later query overwrites (the prover's buff2[I[q]] = pw: the last write wins),
      * changes of I that leave the last-write-wins map unchanged,
    each set computed by its rule above, not by running the verifier."""
    c = opening(oracle, 16, 4, 300)
    o, x, K, trs = c["o"], c["x"], c["K"], c["trs"]
    arr = o[key]
    idxs = sample(arr.size, 600, 1)
    assert len(idxs) == (600 if key in ("reply", "I") else arr.size)
    positions = [int(i[0]) + 4096 * int(i[1]) for i in o["I"]]
    if key == "scalars":
        exempt = [0, 1]
    elif key == "reply":
        per = arr.size // len(arr)
        exempt = [i for i in idxs if i // per in overwritten(positions)]
    elif key == "I":
        exempt = []
        for i in idxs:
            q, j = divmod(i, 2)
            col, row = int(o["I"][q, 0]) ^ (j == 0), int(o["I"][q, 1]) ^ (j == 1)
            if moves_unseen(positions, q, col + 4096 * row):
                exempt.append(i)
    else:
        exempt = []
    got = accepted_after_flips(arr, idxs, lambda: ov.verify_open(o, x, K, trs, c["ends"]))
    assert got == exempt
    ov.verify_open(o, x, K, trs, c["ends"])                      # every change was put back


def test_overwritten_queries_exist_and_their_replies_are_exempt(oracle):
    """the rule's exempt set is not empty at the tamper shape: every entry of every overwritten query's reply is accepted, a last query's is not"""
    c = opening(oracle, 16, 4, 300)
    o = c["o"]
    positions = [int(i[0]) + 4096 * int(i[1]) for i in o["I"]]
    over = sorted(overwritten(positions))
    assert over and len(over) == 300 - len(ov.last_writes(o["I"], 4096))
    per = o["reply"].size // 300
    idxs = [q * per + e for q in over + [299] for e in range(per)]
    got = accepted_after_flips(o["reply"], idxs, lambda: ov.verify_open(o, c["x"], c["K"], c["trs"], c["ends"]))
    assert got == idxs[:-per]


@pytest.mark.parametrize("key", ["q1", "r1", "vr1", "q2", "r2", "vr2", "I", "reply"])
def test_one_bit_changes_of_a_shockwave_proof_are_rejected(oracle, key):
    """(2^12, 8): width 1024, 240 queries, a WHIR proof.  Every entry of q1, r1, vr1, q2, r2 (with the popped challenge behind the view) and vr2,
    every entry of I, 600 seeded entries of reply.  Accepted are exactly
      * the replies of queries whose column a later query asks again (the verifier sums over the distinct columns and reads the last
        reply of each; the prover's replies to one column are equal, so which one it reads is a convention),
      * changes of I that leave the set of distinct columns and the reply read for each unchanged: another query, earlier or later, asks the
        column the query stood at (a shockwave query carries no weight of its own, and that query's reply is the same), and a later query asks
        the column it goes to (were it the last one there, its reply, another column's, would be read),
    by these rules and not by running the verifier; no entry of q1, q2, r1, r2, vr1, vr2 is among them."""
    c = shockwave(oracle, 12, 8)
    sp, x, k = c["sp"], c["x"], c["k"]
    arr = ov.full_r2(sp) if key == "r2" else sp[key]
    if key == "r2":
        assert len(arr) == len(sp["r2"]) + 1
    idxs = sample(arr.size, 600, 2)
    columns = [int(v) for v in sp["I"]]
    if key == "reply":
        per = arr.size // 240
        exempt = [i for i in idxs if i // per in overwritten(columns)]
    elif key == "I":
        assert len(idxs) == 240
        exempt = [i for i in idxs if columns.count(columns[i]) > 1 and (columns[i] ^ 1) in columns[i + 1:]]
        assert exempt
    else:
        exempt = []
    got = accepted_after_flips(arr, idxs, lambda: ov.verify_shockwave(sp, x, k, c["end"]))
    assert got == exempt
    if key == "reply":
        assert overwritten(columns)                                  # 240 queries in 1024 columns: repeated columns are there
    ov.verify_shockwave(sp, x, k, c["end"])


def test_a_failed_whir_check_is_rejected(oracle):
    c = shockwave(oracle, 12, 8)
    sp = c["sp"]
    for i in (0, 1):
        sp["wchecks"][i] = 0
        with pytest.raises(Rejected) as e:
            ov.verify_shockwave(sp, c["x"], c["k"], c["end"])
        sp["wchecks"][i] = 1
        assert e.value.relation == ov.SP_WHIR


@pytest.mark.parametrize("relation,change", [
    (ov.P1_CLAIM, "p1"), (ov.P2_CLAIM, "p2"), (ov.P5_CLAIM, "y1"), (ov.P2_POWERS, "s0"), (ov.P3_CLAIM, "s2"), (ov.P4_CLAIM, "a"),
    (ov.P3_WEIGHTS, "w3"), (ov.P4_EQ, "eq4"),
    (ov.P4_END, "C"), (ov.P5_END, "aggr"), (ov.QUERY_RANGE, "col"), (ov.QUERY_RANGE, "row")])
def test_each_relation_is_named(oracle, relation, change):
    """a change that keeps every round test intact reaches the relation behind it, and the exception carries that relation's name"""
    c = opening(oracle, 16, 4, 300)
    o, x, K, trs = c["o"], c["x"], c["K"], c["trs"]
    cols, R1, logc, R3, off = ov.open_shape(16, K, trs)
    o = dict(o); ends = c["ends"]
    for k in ("poly", "vr", "scalars", "I"):
        o[k] = o[k].copy()
    if change in ("p1", "p2"):                                   # q_0(t) = a t^2 + b t + c -> b + 1, c - r_0: q_0(r_0) stays, the claim moves by 1 - 2 r_0
        at = off[0] if change == "p1" else off[1]
        r0 = fi(o["r"][at])
        q = [fi(v) for v in o["poly"][at]]
        q[1] = ov.fadd(q[1], ov.ONE); q[2] = ov.fsub(q[2], r0)
        o["poly"][at] = np.array(q, np.uint64)
    elif change in ("w3", "eq4"):                                # the two final values doubled and halved: their product stays
        i, j = (2, 1) if change == "w3" else (3, 0)
        o["vr"][i, j] = np.array(ov.fmul(fi(o["vr"][i, j]), (2, 0)), np.uint64)
        o["vr"][i, 1 - j] = np.array(ov.fmul(fi(o["vr"][i, 1 - j]), ((ov.P + 1) // 2, 0)), np.uint64)
    elif change in ("y1", "s0", "s2", "a"):
        o["scalars"][{"s0": 1, "s2": 2, "a": 3, "y1": 4}[change], 1] ^= np.uint64(1)
    elif change in ("C", "aggr"):
        def ends(pc, pa, inner=c["ends"]):
            Cv, Av = inner(pc, pa)
            return (ov.fadd(Cv, ov.ONE), Av) if change == "C" else (Cv, ov.fadd(Av, ov.ONE))
    elif change == "col":
        o["I"][7, 0] = cols
    else:
        o["I"][7, 1] = 2 * trs
    with pytest.raises(Rejected) as e:
        ov.verify_open(o, x, K, trs, ends)
    assert e.value.relation == relation


# ---- binding --------------------------------------------------------------------------------------------------------------------------------------------
def test_an_opening_of_another_polynomial_is_rejected_at_p3s_claim(oracle):
    """committed: poly; opened: poly with one bit of one coefficient changed, over the committed tensor.  The prover's own checks still read
    [1, 1, 1]; the replies (the committed tensor's) are not what P3 was run on"""
    c = opening(oracle, 16, 4, 300, other=True)
    assert c["o"]["checks"].tolist() == [1, 1, 1]
    with pytest.raises(Rejected) as e:
        ov.verify_open(c["o"], c["x"], c["K"], c["trs"], c["ends"])
    assert e.value.relation == ov.P3_CLAIM
    good = opening(oracle, 16, 4, 300)
    assert np.array_equal(good["o"]["I"], c["o"]["I"]) and np.array_equal(good["o"]["reply"], c["o"]["reply"])
