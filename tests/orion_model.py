"""tests/orion_model.py -- the Orion baseline, test_PC(N, 2, K) (src/Our_PC.cpp:28-65 _compute_tensorcode_linear_code, 173-195
commit_standard_orion, 523-602 open_orion_standard, 804-825 the driver; src/PC_utils.cpp:150-166 recursive_prover_orion), restated from the
oracle's pieces (encode_monolithic, MT_commit_Blake, shockwave_commit / shockwave_prove, the field ops) and tests/parity_model.py for the
parity matrix and prove_linear_code_batch, with libc through ctypes.  TEST INFRASTRUCTURE ONLY.

N = 2^n, n even, B = 2^(n/2), Q = min(B, 4096).  The real reference cannot run past its first SHA3 call (inside the first _whir_prove of
shockwave_prove(C_p), in open_parity_matrix); up to there this model is pinned by tests/golden/orion.npz, and it covers what lies behind: the
rest of the parity opening, shockwave_prove(C), the Q^2 paths and the proof size.

Quirks kept as built: r_v[0] is drawn and never used, and no value depends on x; the queried columns are re-encoded in the reference, which is
column I[q] of the tensor bit for bit (asserted in commit's own test); the proof size adds a constant 2^20 F, verifies at positions
(J[j] / 2) B + I[i] / 2 (not the opened (J[j] / 4) 2B + I[i]) and reads an uninitialised `visited`: it is all false here.
"""
import ctypes

import numpy as np

import parity_model as pm
from oracle import pyoracle

MAX_QUERIES = 4096
_libc = ctypes.CDLL(None)


def graphs(orc, n):
    levels, dep, m = {}, 0, n
    while m > 13:
        for kind in (0, 1):
            levels[(dep, kind)] = orc.graph(dep, kind)
        m = int(0.211 * m); dep += 1
    return levels


def shape(N):
    n = N.bit_length() - 1
    assert N == 1 << n and n % 2 == 0
    B = 1 << (n // 2)
    return B, min(B, MAX_QUERIES)


def start(orc, N):
    """test_PC(N, 2, .)'s libc stream of a fresh process up to the commitment: the polynomial, then the graphs of n = B (drawn inside
    commit_standard_orion)"""
    orc.rng_reset()
    poly = orc.generate_randomness(N)
    orc.expander_init_store(shape(N)[0])
    return poly


def tensorcode(orc, poly):
    """_compute_tensorcode_linear_code: T (2B, 2B, 2) row-major and the codeword length"""
    B = shape(poly.shape[0])[0]; S = 2 * B
    T = np.zeros((S, S, 2), np.uint64)
    ln = 0
    for i in range(B):
        T[i], ln = orc.encode_monolithic(poly[i * B:(i + 1) * B])
    for c in range(ln):                                      # columns from ln on hold zero messages: their codewords are zero
        T[:, c] = orc.encode_monolithic(T[:B, c])[0]
    return T, ln


def commit(orc, poly):
    """commit_standard_orion (graphs for n = B drawn): the tensor, MT_commit_Blake over its 4N elements"""
    N = poly.shape[0]; B, Q = shape(N)
    T, ln = tensorcode(orc, poly)
    lv = orc.mt_commit_blake(T.reshape(-1, 2))
    assert lv.shape[0] == 2 * N - 1
    return dict(N=N, B=B, Q=Q, len=ln, T=T, levels=lv, root=lv[-1].copy())


def grid_positions(I, J, cols):
    """open_tree_blake(MT, {I[i], J[j]}, cols) for every pair, i outer: the leaves (J[j] / 4) cols + I[i]"""
    return ((J.astype(np.int64) // 4)[None, :] * cols + I.astype(np.int64)[:, None]).reshape(-1)


def paths_of(levels, n, pos):
    """the sibling paths of the leaves pos from the flat levels over n leaves: (len(pos), log2 n, 32)"""
    pos = np.asarray(pos, np.int64); depth = n.bit_length() - 1
    out = np.zeros((len(pos), depth, 32), np.uint8)
    off, sz = 0, n
    for l in range(depth):
        out[:, l] = levels[off + ((pos >> l) ^ 1)]
        off += sz; sz //= 2
    return out


def open_(orc, C, x, prove=True):
    """open_orion_standard on the commitment C = commit(orc, poly); libc draws in the reference's order.  prove=False stops before the
    shockwave_prove calls (the reference's first SHA3 lies inside the first of them)"""
    B, Q, N = C["B"], C["Q"], C["N"]; S = 2 * B
    l = S.bit_length() - 1; lq = Q.bit_length() - 1
    orc.generate_randomness(1)                                                   # r_v[0] (:540): drawn, its powers feed nothing
    IJ = np.array([_libc.rand() % S for _ in range(2 * Q)], np.uint32)           # (:547-558) interleaved
    I, J = IJ[0::2].copy(), IJ[1::2].copy()
    codewords = np.ascontiguousarray(C["T"][:, I.astype(np.int64)].transpose(1, 0, 2))      # (:560-568)
    arr = codewords.reshape(-1, 2)
    enc_c, lv_c = orc.shockwave_commit(arr, 32)                                  # recursive_prover_orion (src/PC_utils.cpp:150-166)
    PC = pm.commit(orc, B)
    r1 = orc.generate_randomness(l); r2 = orc.generate_randomness(lq)
    P1 = pm.prove_linear_code_batch(orc, codewords, B, r1, r2); P1["r1"] = r1; P1["r2"] = r2
    par = pm.open_(orc, PC, P1["r"], r1, prove=prove)
    out = dict(I=I, J=J, c_root=lv_c[-1].copy(), cp_root=PC["root"], p1=P1, parity=par, checks=par["checks"], P=PC["P"], arr=arr)
    if prove:
        out["sp_c"] = orc.shockwave_prove(arr, enc_c, 32, np.concatenate([P1["r"], r2]), lv_c)
        out["ps"] = proof_size(out, N)
    return out


def paths(C, res, pairs=None):
    """the opened paths: all Q^2 (pairs None), or those of the pair indices i Q + j given"""
    pos = grid_positions(res["I"], res["J"], 2 * C["B"])
    return paths_of(C["levels"], C["N"], pos if pairs is None else pos[np.asarray(pairs, np.int64)])


def grid_ps(I, J, B, N):
    """(:588-595) per pair 2 F and verify_claim_opt_blake at (J[j] / 2) B + I[i] / 2, i outer, `visited` all false at the start.  A position
    met before adds nothing, so the walk runs over the distinct positions in order of first appearance"""
    Q = len(I)
    pos = ((J.astype(np.int64) // 2)[None, :] * B + (I.astype(np.int64) // 2)[:, None]).reshape(-1)
    _, first = np.unique(pos, return_index=True)
    order = pos[np.sort(first)]
    depth = N.bit_length() - 1
    return Q * Q * 2 * 16.0 / 1024.0 + pyoracle._path_ps(N, depth, order)


def proof_size(res, N):
    """the ps (KB) open_orion_standard accumulates from 0: prove_linear_code_batch, open_parity_matrix, shockwave_prove(C) (:570), the
    constant (:571), the grid (:588-595).  Every term is a multiple of 1/64: the sum is exact in any order"""
    B, Q = shape(N); S = 2 * B
    ps = pyoracle._sc_ps(S.bit_length() - 1)
    ps += pm.open_proof_size(res["parity"], res["P"])
    ps += pyoracle._shockwave_ps(res["sp_c"], Q * S, 32)
    ps += (1 << 20) * 16.0 / 1024.0
    return ps + grid_ps(res["I"], res["J"], B, N)


def transcript(orc, C, x, T, peek, prove=True):
    """the opening again with the record sequence (x, k, mimc(x, k)) it implies, in the reference's order: P1 (seeded with r1's last entry), then
    the parity opening's as tests/test_parity_matrix.py lays them out (T: its Transcript, peek: its peek_randomness)"""
    seen = []
    real = orc.mul_tree

    def spy(inp, previous_r, prev_x=None):
        seen.append(peek(orc, 2))
        return real(inp, previous_r, prev_x)
    orc.mul_tree = spy
    try:
        res = open_(orc, C, x, prove=prove)
    finally:
        del orc.mul_tree
    p1, par = res["p1"], res["parity"]
    T.sumcheck(p1["r1"][-1], p1["poly"], p1["r"], p1["vr"], p1["fin"], False)
    T.tree(par["t1"], seen[0][-1]); T.tree(par["t2"], seen[1][-1])
    T.sumcheck(pm.Fi(321), par["p2"]["poly"], par["p2"]["r"], par["p2"]["vr"], par["p2"]["fin"], True)
    T.sumcheck(pm.Fi(321), par["p3"]["poly"], par["p3"]["r"], par["p3"]["vr"], par["p3"]["fin"], False)
    T.sumcheck(pm.Fi(321), par["p4"]["poly"], par["p4"]["r"], par["p4"]["vr"], par["p4"]["fin"], False)
    if prove:
        T.shockwave_head(par["sp_p"])
    return res, T.records()


# ---- computed once per session and shared by tests/test_orion_model_cpu.py and tests/test_orion.py; nobody writes into what these return --------
_CACHE = {}


def begin(orc, logn):
    """the libc stream of a fresh process up to the call of open_orion_standard: polynomial, graphs, x"""
    poly = start(orc, 1 << logn)
    return poly, orc.generate_randomness(logn)


def model_commit(orc, logn):
    if logn not in _CACHE:
        _CACHE[logn] = commit(orc, start(orc, 1 << logn))
    return _CACHE[logn]


def model_open(orc, logn, T, peek):
    """the model's opening with its record sequence (T, peek: tests/test_parity_matrix.py's Transcript and peek_randomness)"""
    if (logn, "open") not in _CACHE:
        C = model_commit(orc, logn)
        _, x = begin(orc, logn)
        res, rec = transcript(orc, C, x, T(orc), peek)
        _CACHE[(logn, "open")] = dict(x=x, open=res, records=rec)
    return _CACHE[(logn, "open")]
