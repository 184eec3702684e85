"""tests/brakingbase_model.py -- the Braking base baseline, test_PC(N, 5, K) (src/Our_PC.cpp:114-144 commit_brakingbase, 238-256
_aggregate_brakingbase, 355-429 open_brakingbase, 827-842 the driver; src/PC_utils.cpp:389-394 recursive_prover_brakingbase), restated from the
oracle's pieces (encode_monolithic, BLAKE3, precompute_beta, shockwave_commit / shockwave_prove, prove_linear_code, the field ops) and
tests/parity_model.py for the parity matrix, with libc through ctypes.  TEST INFRASTRUCTURE ONLY.

The real reference cannot run past its first SHA3 call (inside the first _whir_prove of shockwave_prove(C_p), in open_parity_matrix); up to there
this model is pinned by tests/golden/brakingbase.npz -- the commitment, I, the paths, the roots of C_c, C_p, C_w and the mimc transcript record
for record -- and it covers what lies behind: the rest of the parity opening and shockwave_prove(C_c, P1.randomness[0]).

Quirks kept as built: r_v[0] is drawn and never used; every opening path is leaf 0's (open_tree_blake(MT, {0, I[q]}, 0) takes leaf
(I[q] / 4) * 0 + 0); parents of both trees are H(left | left) (left_left_quirk = 1; 0 gives conventional trees, which the reference never
builds: the model implements both so that the general column digest of the device has something to be checked against).
"""
import ctypes

import numpy as np

import parity_model as pm
from oracle import pyoracle

QUERIES = 2935
_libc = ctypes.CDLL(None)


def graphs(orc, n):
    levels, dep, m = {}, 0, n
    while m > 13:
        for kind in (0, 1):
            levels[(dep, kind)] = orc.graph(dep, kind)
        m = int(0.211 * m); dep += 1
    return levels


def start(orc, N, K):
    """test_PC(N, 5, K)'s libc stream of a fresh process up to the commitment: the polynomial, then the graphs of n = trs = N / K"""
    orc.rng_reset()
    poly = orc.generate_randomness(N)
    orc.expander_init_store(N // K)
    return poly


def _parents(orc, h, quirk):
    left = h[0::2]
    return orc.blake3_64(np.concatenate([left, left if quirk else h[1::2]], axis=1))


def column_digests(orc, T, quirk):
    """MT_commit_Blake of every column of T (K, W, 2): leaves H(rows 4l .. 4l + 3), then create_tree_blake's parents"""
    K, W = T.shape[0], T.shape[1]
    h = orc.blake3_64(np.ascontiguousarray(T.transpose(1, 0, 2)).view(np.uint8).reshape(-1, 64)).reshape(W, K // 4, 32)
    while h.shape[1] > 1:
        h = _parents(orc, h.reshape(-1, 32), quirk).reshape(W, -1, 32)
    return h[:, 0]


def tree(orc, leaves, quirk):
    """create_tree_blake over the leaves: the flat levels, leaves first"""
    out = [leaves]
    while out[-1].shape[0] > 1:
        out.append(_parents(orc, out[-1], quirk))
    return np.concatenate(out)


def commit(orc, poly, K, quirk=1):
    """commit_brakingbase: tensor[0][i] = encode_monolithic(row i), the column digests, the tree over them (graphs for n = trs drawn)"""
    N = poly.shape[0]; trs = N // K
    rows = [orc.encode_monolithic(poly[i * trs:(i + 1) * trs]) for i in range(K)]
    T = np.stack([r[0] for r in rows])
    lv = tree(orc, column_digests(orc, T, quirk), quirk)
    return dict(N=N, K=K, trs=trs, len=rows[0][1], T=T, levels=lv, root=lv[-1].copy(), quirk=quirk)


def open_(orc, C, x, prove=True):
    """open_brakingbase on the commitment C = commit(orc, poly, K); libc draws in the reference's order.  prove=False stops the parity opening
    and the model before the shockwave_prove calls (the reference's first SHA3 lies inside the first of them)"""
    K, trs = C["K"], C["trs"]; W = 2 * trs
    lk = K.bit_length() - 1; l = W.bit_length() - 1
    beta = orc.precompute_beta(x[:lk])
    orc.generate_randomness(1)                                                   # r_v[0] (:374): drawn, its powers feed nothing
    aggr = np.zeros((trs, 2), np.uint64)                                         # _aggregate_brakingbase (:238-256)
    for i in range(K):
        aggr = orc.f_add(aggr, orc.f_mul(np.broadcast_to(beta[i], (trs, 2)), C["T"][i, :trs]))
    codeword, _ = orc.encode_monolithic(aggr)
    enc_c, lv_c = orc.shockwave_commit(codeword, 32)
    I = np.array([_libc.rand() % W for _ in range(QUERIES)], np.uint32)          # (:382-385)
    reply = np.ascontiguousarray(C["T"][:, I.astype(np.int64)].transpose(1, 0, 2))
    off, sz, path = 0, W, []
    while sz > 1:                                                                # leaf 0's path: the sibling of node 0 on every level
        path.append(C["levels"][off + 1]); off += sz; sz //= 2
    paths = np.broadcast_to(np.stack(path), (QUERIES, l, 32)).copy()
    PC = pm.commit(orc, trs)                                                     # recursive_prover_brakingbase (src/PC_utils.cpp:389-394)
    r1 = orc.generate_randomness(l)
    P1 = orc.prove_linear_code(codeword, trs, r1); P1["r1"] = r1
    par = pm.open_(orc, PC, P1["r"], r1, prove=prove)
    out = dict(I=I, reply=reply, paths=paths, aggr=aggr, cc_root=lv_c[-1].copy(), cp_root=PC["root"], p1=P1, parity=par, checks=par["checks"], P=PC["P"])
    if prove:
        out["sp_c"] = orc.shockwave_prove(codeword, enc_c, 32, P1["r"], lv_c)
        out["ps"] = proof_size(out, K, trs)
    return out


def proof_size(res, K, trs):
    """the ps (KB) open_brakingbase accumulates from 0: the replies (:393), prove_linear_code, open_parity_matrix, shockwave_prove(C_c),
    verify_claim_opt_blake fed with I[q] (:422-424).  Every term is a multiple of 1/64: the sum is exact in any order"""
    W = 2 * trs; l = W.bit_length() - 1
    ps = QUERIES * K * 16.0 / 1024.0
    ps += pyoracle._sc_ps(l)
    ps += pm.open_proof_size(res["parity"], res["P"])
    ps += pyoracle._shockwave_ps(res["sp_c"], W, 32)
    return ps + pyoracle._path_ps(W, l, res["I"])


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
