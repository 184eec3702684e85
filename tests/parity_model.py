"""tests/parity_model.py -- commit_parity_matrix / open_parity_matrix / prove_linear_code_batch (src/sumcheck.cpp:2622-2885, 3201-3221) restated
from the oracle's primitives (graph, precompute_beta, mul_tree, sumcheck3, sumcheck2, evaluate_vector, shockwave_commit, shockwave_prove, the
field ops) with libc through ctypes.  TEST INFRASTRUCTURE ONLY.

The real reference cannot run past its first SHA3 call (inside the first _whir_prove of shockwave_prove(C_p)); up to there this model is pinned
record for record by tests/golden/parity_matrix.npz, and it covers what lies behind.

INDEX PADDING = 0: open_parity_matrix reads access_idx1[i] / access_idx2[i] for m <= i < P (:2756-2763), past the vectors' size but inside the
capacity push_back left.  The defined result is the reference's under a zero-filling allocator (the fixture's MALLOC_PERTURB_=255 run).

Two layouts of the public witness, both as written: commit_parity_matrix puts idx2 at offset m (:2696-2698), open_parity_matrix at offset P
for P4 (:2850-2852); shockwave_prove(C_p, P4.randomness) then opens the commit layout at P4's point.
"""
import ctypes
import numpy as np

P61 = (1 << 61) - 1
_libc = ctypes.CDLL(None)
_libc.random.restype = ctypes.c_long


def Fi(v):
    return np.array([int(v) % P61, 0], np.uint64)


def ints_to_F(a):
    out = np.zeros((len(a), 2), np.uint64); out[:, 0] = a
    return out


def f_mul(a, b):
    a = [int(x) for x in a]; b = [int(x) for x in b]
    return np.array([(a[0] * b[0] - a[1] * b[1]) % P61, (a[0] * b[1] + a[1] * b[0]) % P61], np.uint64)


def f_add(a, b):
    return np.array([(int(a[0]) + int(b[0])) % P61, (int(a[1]) + int(b[1])) % P61], np.uint64)


def f_sub(a, b):
    return np.array([(int(a[0]) - int(b[0])) % P61, (int(a[1]) - int(b[1])) % P61], np.uint64)


ONE = Fi(1)


def access_lists(orc, n):
    """generate_access_idx (:2622-2669) over the graphs orc.expander_init_store(n) left: idx1, idx2 (int64), weight (F)"""
    i1, i2, w = [], [], []

    def rec(off, m, dep, lvl):
        if m <= 13:
            return m
        C, D = orc.graph(dep, 0), orc.graph(dep, 1)
        assert C["L"] == m
        R, d = C["R"], C["degree"]
        i1.append(C["nbr"] + lvl); i2.append(np.repeat(np.arange(m, dtype=np.int64) + off, d)); w.append(C["w"])
        i1.append(lvl + np.arange(R, dtype=np.int64)); i2.append(np.arange(R, dtype=np.int64) + off + m); w.append(np.tile(Fi(-1), (R, 1)))
        L = rec(off + m, R, dep + 1, lvl + R)
        assert D["L"] == L
        R2, d = D["R"], D["degree"]
        i1.append(D["nbr"] + lvl); i2.append(np.repeat(np.arange(L, dtype=np.int64) + off + m, d)); w.append(D["w"])
        i1.append(lvl + np.arange(R2, dtype=np.int64)); i2.append(np.arange(R2, dtype=np.int64) + off + m + L); w.append(np.tile(Fi(-1), (R2, 1)))
        return m + L + R2

    rec(0, n, 0, 0)
    return np.concatenate(i1), np.concatenate(i2), np.concatenate(w)


def lists(orc, n):
    """the lists as the device object holds them: padded to P with zeros; counters 1-based; final access counts of the 2n cells"""
    i1, i2, w = access_lists(orc, n)
    m = len(i1); P = 1
    while P < m:
        P *= 2
    S = 2 * n
    a1 = np.zeros(S, np.int64); a2 = np.zeros(S, np.int64); c1 = np.zeros(m, np.int64); c2 = np.zeros(m, np.int64)
    for i in range(m):
        a1[i1[i]] += 1; c1[i] = a1[i1[i]]
        a2[i2[i]] += 1; c2[i] = a2[i2[i]]
    pad = lambda v: np.concatenate([v, np.zeros(P - m, v.dtype)])  # noqa: E731
    return dict(n=n, m=m, P=P, idx1=pad(i1), idx2=pad(i2), cnt1=pad(c1), cnt2=pad(c2), weight=np.concatenate([w, np.zeros((P - m, 2), np.uint64)]),
                acc1=ints_to_F(a1), acc2=ints_to_F(a2))


def public_witness(ls, off2):
    """8P F: idx1 at 0, idx2 at off2 (m: the commit's layout, P: the open's), cnt1 at 2P, cnt2 at 3P, weight at 4P, acc1 at 5P, acc2 at 5P + 2n"""
    m, P, S = ls["m"], ls["P"], 2 * ls["n"]
    assert 4 * P < 5 * P + 2 * S <= 8 * P
    pw = np.zeros((8 * P, 2), np.uint64)
    pw[:m, 0] = ls["idx1"][:m]; pw[off2:off2 + m, 0] = ls["idx2"][:m]
    pw[2 * P:3 * P, 0] = ls["cnt1"]; pw[3 * P:4 * P, 0] = ls["cnt2"]; pw[4 * P:5 * P] = ls["weight"]
    pw[5 * P:5 * P + S] = ls["acc1"]; pw[5 * P + S:5 * P + 2 * S] = ls["acc2"]
    return pw


def commit(orc, n):
    """commit_parity_matrix(n): the lists and C_p = shockwave_commit(public_witness, 16)"""
    ls = lists(orc, n)
    pw = public_witness(ls, ls["m"])
    enc, lv = orc.shockwave_commit(pw, 16)
    return dict(ls, pw=pw, enc=enc, levels=lv, root=lv[-1].copy())


def _scal_vec(orc, s, v):
    return orc.f_mul(np.broadcast_to(s, v.shape), v)


def open_(orc, C, r1, r2, prove=True):
    """open_parity_matrix(r1, r2, n) on the commitment C = commit(orc, n); libc draws in the reference's order"""
    n, m, P = C["n"], C["m"], C["P"]; S = 2 * n
    L = P.bit_length() - 1; l = S.bit_length() - 1
    beta1, beta2 = orc.precompute_beta(r1), orc.precompute_beta(r2)
    betas1, betas2 = beta1[C["idx1"]].copy(), beta2[C["idx2"]].copy()
    betas1[m:] = 0; betas2[m:] = 0
    betas12 = np.concatenate([betas1, betas2])
    encw, lvw = orc.shockwave_commit(betas12, 16)
    a, b = Fi(_libc.random()), Fi(_libc.random())
    ones = np.tile(ONE, (P, 1))
    rows = []
    for idx, cnt, bt in ((C["idx1"], C["cnt1"], betas1), (C["idx2"], C["cnt2"], betas2)):
        hi = orc.f_add(orc.f_add(_scal_vec(orc, a, ints_to_F(idx)), _scal_vec(orc, b, ints_to_F(cnt))), orc.f_add(bt, ones))
        rows += [orc.f_sub(hi, np.broadcast_to(b, hi.shape)), hi]
    t1 = orc.mul_tree(np.stack(rows), Fi(21))
    ind = t1["final_r"][:L]
    eq = orc.precompute_beta(ind)[:m]
    dot = lambda v: np.array([int(x) % P61 for x in orc.f_mul(eq, v[:m]).astype(object).sum(axis=0)], np.uint64)  # noqa: E731
    partial = np.stack([dot(ints_to_F(C[k])) for k in ("idx1", "idx2", "cnt1", "cnt2")] + [dot(C["weight"]), dot(betas1), dot(betas2)])
    ai = _scal_vec(orc, a, ints_to_F(np.arange(S))); oneS = np.tile(ONE, (S, 1))
    rows = []
    for bt, acc in ((beta1, C["acc1"]), (beta2, C["acc2"])):
        lo = orc.f_add(orc.f_add(ai, bt), oneS)
        rows += [lo, orc.f_add(_scal_vec(orc, b, acc), lo)]
    t2 = orc.mul_tree(np.stack(rows), Fi(21))
    y1a, y2a = orc.evaluate_vector(C["acc1"], ind[:l]), orc.evaluate_vector(C["acc2"], ind[:l])
    p5 = f_add(f_mul(y1a, f_sub(ONE, ind[l])), f_mul(y2a, ind[l]))
    for i in range(l + 1, L):
        p5 = f_mul(p5, f_sub(ONE, ind[i]))
    P2 = orc.sumcheck3(C["weight"], betas1, betas2, Fi(321))
    r, a_ = Fi(_libc.random()), Fi(_libc.random())
    y1 = f_add(f_mul(f_sub(ONE, r), partial[5]), f_mul(r, partial[6]))
    y2 = f_add(f_mul(f_sub(ONE, r), P2["vr"][1]), f_mul(r, P2["vr"][2]))
    eqs = lambda pa, pb: orc.f_add(orc.precompute_beta(pa), _scal_vec(orc, a_, orc.precompute_beta(pb)))  # noqa: E731
    P3 = orc.sumcheck2(eqs(np.concatenate([ind, r[None]]), np.concatenate([P2["r"], r[None]])), betas12, Fi(321))
    checks = np.zeros(2, np.int32)
    checks[0] = int(np.array_equal(orc.claim_of(P3["poly"][0]), f_add(y1, f_mul(a_, y2))))
    pw2 = public_witness(C, P)
    pad = orc.generate_randomness(3)
    y1 = orc.evaluate_vector(np.concatenate([partial[:5], p5[None], np.zeros((2, 2), np.uint64)]), pad)
    sel = np.array([[0, 0], [0, 0], [1, 0]], np.uint64)
    P4 = orc.sumcheck2(eqs(np.concatenate([ind, pad]), np.concatenate([P2["r"], sel])), pw2, Fi(321))
    checks[1] = int(np.array_equal(orc.claim_of(P4["poly"][0]), f_add(y1, f_mul(a_, P2["vr"][0]))))
    out = dict(t1=t1, t2=t2, p2=P2, p3=P3, p4=P4, cw_root=lvw[-1].copy(), scalars=np.stack([a, b, r, a_]), partial=partial, acc_y=np.stack([y1a, y2a]),
               checks=checks, betas12=betas12)
    if prove:
        out["sp_p"] = orc.shockwave_prove(C["pw"], C["enc"], 16, P4["r"], C["levels"])
        out["sp_w"] = orc.shockwave_prove(betas12, encw, 16, P3["r"], lvw)
    return out


def prove_linear_code_batch(orc, codewords, n, r1, r2):
    """prove_linear_code_batch (:3201-3221) with the challenges given: codewords (count, len <= 2n, 2)"""
    S = 2 * n
    A, _ = orc.evaluate_parity_matrix(orc.precompute_beta(r1), n)
    beta2 = orc.precompute_beta(r2)
    B = np.zeros((S, 2), np.uint64)
    for i in range(codewords.shape[0]):
        B[:codewords.shape[1]] = orc.f_add(B[:codewords.shape[1]], _scal_vec(orc, beta2[i], codewords[i]))
    return orc.sumcheck2(A, B, r1[-1])


def open_proof_size(res, P):
    """the ps (KB) open_parity_matrix accumulates, piece by piece: every layer of both trees and P2 as _generate_3product_sumcheck_proof counts
    them (5 F per round and 3 at the end, src/sumcheck.cpp:2031, 2048), P3 and P4 (:2431, 2449), the two shockwave_prove calls"""
    from oracle import pyoracle
    F16 = 16.0 / 1024.0
    L = P.bit_length() - 1
    ps = 0.0
    for t in ("t1", "t2"):
        for k in range(int(res[t]["layers"][0])):
            ps += ((2 + k) * 5 + 3) * F16
    ps += (L * 5 + 3) * F16
    ps += pyoracle._sc_ps(L + 1); ps += pyoracle._sc_ps(L + 3)
    ps += pyoracle._shockwave_ps(res["sp_p"], 8 * P, 16); ps += pyoracle._shockwave_ps(res["sp_w"], 2 * P, 16)
    return ps
