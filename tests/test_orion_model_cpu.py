"""tests/orion_model.py held to tests/golden/orion.npz -- the REAL reference's own test_PC(2^n, 2, 128) as far as it can run
(scripts/gen_orion_golden.py) -- record for record, and to the oracle's tree for the opening paths, which the reference never reaches.
CPU only."""
import hashlib
import os

import numpy as np
import pytest

import orion_model as om
from test_parity_matrix import Transcript, peek_randomness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "orion.npz")
SHAPES = (14, 16, 18, 20)


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def level_dgs(flat, n):
    out, off, sz = [], 0, n
    while sz >= 1:
        out.append(dg(flat[off:off + sz])); off += sz; sz //= 2
    return np.stack(out)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD, allow_pickle=False))
    assert tuple(int(v) for v in g["shapes"]) == SHAPES
    assert os.path.getsize(GOLD) < 400 << 10
    return g


@pytest.mark.parametrize("logn", SHAPES)
def test_model_commit_matches_reference(oracle, gold, logn):
    C = om.model_commit(oracle, logn)
    k = "_%d" % logn; B = C["B"]
    assert np.array_equal(C["root"], gold["root" + k])
    assert np.array_equal(level_dgs(C["levels"], C["N"]), gold["level_dg" + k])
    assert np.array_equal(C["levels"][gold["leaves_idx" + k]], gold["leaves_s" + k])
    assert np.array_equal(dg(C["T"]), gold["T_dg" + k])
    assert np.array_equal(C["T"][:, gold["cols_idx" + k]].transpose(1, 0, 2), gold["cols" + k])
    # every entry outside the codewords is zero, and the reference's re-encode of a queried column's message half is that column
    assert not C["T"][:, C["len"]:].any() and not C["T"][C["len"]:].any() and C["T"][B:C["len"], B:C["len"]].any()
    om.start(oracle, 1 << logn)                              # the commitment may come from the cache: the oracle's graphs are whatever ran last
    for c in (0, B - 1, B, C["len"] - 1):
        assert np.array_equal(oracle.encode_monolithic(C["T"][:B, c])[0], C["T"][:, c])


@pytest.mark.parametrize("logn", SHAPES)
def test_model_open_matches_reference(oracle, gold, logn):
    """x, I, J, the three inner roots, and the transcript record for record up to the reference's first SHA3 call: P1, both multiplication trees,
    P2, P3, P4 and the two sumchecks of shockwave_prove(C_p)"""
    k = "_%d" % logn
    M = om.model_open(oracle, logn, Transcript, peek_randomness)
    res, rec, want = M["open"], M["records"], gold["transcript" + k]
    assert np.array_equal(M["x"], gold["x" + k])
    assert np.array_equal(res["I"], gold["I" + k]) and np.array_equal(res["J"], gold["J" + k])
    assert np.array_equal(res["c_root"], gold["c_root" + k]) and np.array_equal(res["cp_root"], gold["cp_root" + k])
    assert np.array_equal(res["parity"]["cw_root"], gold["cw_root" + k]) and res["P"] == int(gold["P" + k][0])
    assert rec.shape == want.shape, (rec.shape, want.shape)
    bad = np.nonzero((rec != want).any(axis=1))[0]
    assert not len(bad), "first differing record: %d" % bad[0]
    assert res["checks"].tolist() == [1, 1]
    assert np.array_equal(oracle.claim_of(res["p1"]["poly"][0]), np.zeros(2, np.uint64)), "genuine codewords: the claimed sum is zero"


@pytest.mark.parametrize("logn", SHAPES)
def test_model_paths_are_the_oracles(oracle, logn):
    """pairs of the grid -- the corners, and a sample -- against the oracle's open_tree_blake(MT, {I[i], J[j]}, 2B) on the model's levels"""
    C = om.model_commit(oracle, logn)
    res = om.model_open(oracle, logn, Transcript, peek_randomness)["open"]
    Q = C["Q"]
    pairs = np.concatenate([[0, Q - 1, Q * (Q - 1), Q * Q - 1], np.random.default_rng(logn).integers(0, Q * Q, 60)])
    got = om.paths(C, res, pairs)
    for p, path in zip(pairs, got):
        i, j = int(p) // Q, int(p) % Q
        assert np.array_equal(path, oracle.open_tree_blake(C["levels"], C["N"], int(res["I"][i]), int(res["J"][j]), 2 * C["B"])), (i, j)


def test_proof_size_walk_over_distinct_positions_is_the_full_walk():
    """grid_ps walks the distinct positions in order of first appearance; the reference walks all Q^2: equal, on a grid with many repeats"""
    from oracle import pyoracle
    g = np.random.default_rng(5)
    B, N = 16, 256
    I = g.integers(0, 2 * B, 16).astype(np.uint32); J = g.integers(0, 2 * B, 16).astype(np.uint32)
    pos = [(int(j) // 2) * B + int(i) // 2 for i in I for j in J]
    assert om.grid_ps(I, J, B, N) == len(pos) * 32.0 / 1024.0 + pyoracle._path_ps(N, 8, pos)
