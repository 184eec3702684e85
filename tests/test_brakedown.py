"""The Brakedown comparison baseline, test_PC(N, 3, K) (reference src/Our_PC.cpp:197-236 commit_standard_brakedown, 432-520
open_brakedown_standard, 794-805 the driver).

Fixtures: tests/golden/brakedown_2e<n>.npz, recorded from the real reference by scripts/gen_brakedown_golden.py.  Under the reference's
left|left tree (parent = H(left | left)) level 0 depends only on rows 0..3 of the encoded matrix and the root only on column 0, so a matching
root proves little: the tests also pin every level, the whole encoded matrix, the replies, the aggregates and the paths.

CPU: the fixtures agree with the oracle.  GPU: the rows-innermost encode (hobbit_encode_interleaved) against hobbit_encode_batch and the
oracle, commit and open against the fixtures, host/test_pc end to end, the size limits.
"""
import ctypes
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest

from adversarial import families, graphs_from, set_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
P = (1 << 61) - 1
QUERIES = 2900
FULL = (20, 21, 22, 24)


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def shape(logn):
    B = 1 << (logn // 2 + 6) if logn % 2 == 0 else 1 << ((logn - 1) // 2 + 6)
    return B, (1 << logn) // B


def gold(logn):
    return dict(np.load(os.path.join(GOLD, "brakedown_2e%d.npz" % logn)))


def level_dgs(flat, W):
    out, off, sz = [], 0, W
    while sz >= 1:
        out.append(dg(flat[off:off + sz])); off += sz; sz //= 2
    return np.stack(out)


def column_digests(oracle, T4, rows):
    """MT_commit_Blake of every column under the left|left quirk: leaf 0 = H(rows 0..3), re-hashed log2(rows / 4) times"""
    h = oracle.blake3_64(np.ascontiguousarray(T4.transpose(1, 0, 2)).view(np.uint8).reshape(-1, 64))
    for _ in range((rows // 4).bit_length() - 1):
        h = oracle.blake3_64(np.concatenate([h, h], axis=1))
    return h


def verify_ps(I, W):
    """verify_claim_opt_blake's accounting (src/merkle_tree.cpp:326-361), fed with I[q], from 0"""
    depth = W.bit_length() - 1
    visited = set(); ps = 0.0
    for p in I:
        pe = W + int(p)
        for _ in range(depth):
            if (pe ^ 1) in visited:
                break
            visited.add(pe ^ 1); pe //= 2; visited.add(pe)
            ps += 32.0 / 1024.0
    return ps


def draws(oracle, logn):
    """test_PC(2^n, 3, K)'s libc sequence through the oracle: poly, the graphs of n = B, x, r (rows x random()), I (2900 x rand() % 2B)"""
    B, rows = shape(logn)
    oracle.rng_reset()
    poly = oracle.generate_randomness(1 << logn)
    oracle.expander_init_store(B)
    x = oracle.generate_randomness(logn)
    libc = ctypes.CDLL(None); libc.random.restype = ctypes.c_long
    r = np.zeros((rows, 2), np.uint64); r[:, 0] = [libc.random() for _ in range(rows)]
    I = np.array([libc.rand() % (2 * B) for _ in range(QUERIES)], np.uint64)
    return poly, x, r, I


# ---- CPU: the fixtures against the oracle ---------------------------------------------------------
def test_shape_limits():
    from __graft_entry__ import load_package, build_hip
    build_hip()
    hb = load_package()
    assert hb.Hobbit.brakedown_shape(1 << 20) == (1 << 16, 16)
    assert hb.Hobbit.brakedown_shape(1 << 21) == (1 << 16, 32)
    assert hb.Hobbit.brakedown_shape(1 << 28) == (1 << 20, 256)
    assert hb.Hobbit.brakedown_shape(1 << 29) == (1 << 20, 512)
    assert hb.Hobbit.brakedown_shape(1 << 16) == (1 << 14, 4)
    for N in (1 << 15, 1 << 30, 3 << 20):
        with pytest.raises(hb.HobbitError):
            hb.Hobbit.brakedown_shape(N)


@pytest.mark.parametrize("logn", FULL)
def test_fixture_follows_from_oracle(oracle, logn):
    """level 0 = the oracle's encode of rows 0..3 then BLAKE3; the tree, I, r, the aggregates, the sampled entries and replies, and ps follow
    from the draws"""
    g = gold(logn)
    B, rows = shape(logn); W = 2 * B
    assert int(g["B"][0]) == B and int(g["rows"][0]) == rows
    poly, x, r, I = draws(oracle, logn)
    assert np.array_equal(I.astype(np.uint32), g["I"]) and np.array_equal(r, g["r"]) and np.array_equal(x, g["x"])
    need = sorted(set(range(4)) | set(int(i) for i in g["ent_i"]) | set(int(i) for i in g["ri"]))
    T = {}
    for i in need:
        d, ln = oracle.encode_monolithic(poly[i * B:(i + 1) * B])
        T[i] = d
    leaves = column_digests(oracle, np.stack([T[i] for i in range(4)]), rows)
    assert np.array_equal(leaves[g["leaves_idx"]], g["leaves_s"])
    lv = oracle.create_tree_blake(leaves)
    assert np.array_equal(level_dgs(lv, W), g["level_dg"]) and np.array_equal(lv[-1], g["root"])
    assert np.array_equal(np.stack([T[int(i)][int(c)] for i, c in zip(g["ent_i"], g["ent_c"])]), g["ent"])
    assert np.array_equal(np.stack([T[int(i)][int(I[q])] for q, i in zip(g["rq"], g["ri"])]), g["reply_s"])
    # every path is leaf 0's (open_tree_blake(MT, {0, I[q]}, 0) takes (I[q]/4)*0 + 0): sibling of node 0 on every level
    off, sz, want = 0, W, []
    while sz > 1:
        want.append(lv[off + 1]); off += sz; sz //= 2
    assert np.array_equal(np.stack(want), g["path"])
    lr = rows.bit_length() - 1
    beta = oracle.precompute_beta(x[:lr])
    ab = np.zeros((B, 2), np.uint64); ar = np.zeros((B, 2), np.uint64)
    for i in range(rows):
        row = poly[i * B:(i + 1) * B]
        ab = oracle.f_add(ab, oracle.f_mul(np.broadcast_to(beta[i], (B, 2)), row))
        ar = oracle.f_add(ar, oracle.f_mul(np.broadcast_to(r[i], (B, 2)), row))
    assert np.array_equal(dg(ab), g["aggr_beta_dg"]) and np.array_equal(dg(ar), g["aggr_r_dg"])
    assert np.array_equal(ab[g["aj"]], g["aggr_beta_s"]) and np.array_equal(ar[g["aj"]], g["aggr_r_s"])
    ps_paths = verify_ps(I, W)
    assert ps_paths == float(g["ps_paths"][0])
    assert float(g["ps"][0]) == ps_paths + QUERIES * rows * 16 / 1024.0 + (2 * B * 16) // 1024


def test_fixture_2e28_root_from_oracle(oracle):
    """the 2^28 commitment's root is column 0's digest re-hashed (left|left): column 0 of the encoded matrix is poly[0], poly[B], ... (the
    systematic part), so the oracle gets it from the first 4B draws"""
    g = gold(28)
    B, rows = shape(28)
    oracle.rng_reset()
    poly = oracle.generate_randomness(3 * B + 1)
    col0 = np.stack([poly[i * B] for i in range(4)])[None]
    assert np.array_equal(col0[0], g["cols"][0][:4])
    h = column_digests(oracle, col0.transpose(1, 0, 2), rows)
    assert np.array_equal(h[0], g["leaves_s"][0])
    for _ in range((2 * B).bit_length() - 1):
        h = oracle.blake3_64(np.concatenate([h, h], axis=1))
    assert np.array_equal(h[0], g["root"])


# ---- GPU -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


WEIGHTS = {"drawn": None, "2^32-1": [(1 << 32) - 1, 0], "full_p-1": [P - 1, P - 1]}


def _messages(n, rows, seed):
    from oracle.pyoracle import splitmix_field
    x = splitmix_field(n * rows, seed).reshape(rows, n, 2)
    fam = families(n, seed=seed)
    for k, name in enumerate(fam):
        if k < rows:
            x[k] = fam[name]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("n", [64, 1000, 4096, 8192, 16384])
def test_encode_interleaved_matches_encode_batch(hb, oracle, n, wname):
    """bit-identical to hobbit_encode_batch for every rows in {1, 4, 16, 256}, out of place and in place; the first rows are the adversarial
    families (tests/adversarial.py) that drive the lazy sums to their bounds"""
    oracle.rng_reset(); oracle.expander_init_store(n)
    lv = graphs_from(oracle, n)
    if WEIGHTS[wname] is not None:
        lv = set_weights(oracle, lv, WEIGHTS[wname])
    hb.upload_graphs(n, lv)
    for rows in (1, 4, 16, 256):
        x = _messages(n, rows, seed=n + rows)
        want = hb.encode_monolithic(x)                              # (rows, 2n, 2)
        for in_place in (False, True):
            got = hb.encode_interleaved(np.ascontiguousarray(x.transpose(1, 0, 2)), in_place=in_place)
            assert np.array_equal(got.transpose(1, 0, 2), want), (n, wname, rows, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,rows", [(16, 16), (20, 4)])
def test_encode_interleaved_matches_oracle(hb, oracle, logn, rows):
    n = 1 << logn
    oracle.rng_reset(); oracle.expander_init_store(n)
    hb.upload_graphs(n, graphs_from(oracle, n))
    x = _messages(n, rows, seed=logn)
    got = hb.encode_interleaved(np.ascontiguousarray(x.transpose(1, 0, 2)))
    for i in range(rows):
        want, ln = oracle.encode_monolithic(x[i])
        assert np.array_equal(got[:ln, i], want[:ln]), (logn, i)
        assert not got[ln:, i].any()


def _commit(hb, oracle, logn, quirk=1):
    poly, x, r, I = draws(oracle, logn)
    B, rows = shape(logn)
    hb.upload_graphs(B, graphs_from(oracle, B))
    return hb.brakedown_commit(poly, quirk=quirk), poly, x, r, I


@pytest.mark.gpu
@pytest.mark.parametrize("logn", FULL)
def test_commit_open_match_reference(hb, oracle, logn):
    g = gold(logn)
    c, poly, x, r, I = _commit(hb, oracle, logn)
    B, rows = shape(logn); W = 2 * B
    assert (c.B, c.rows) == (B, rows)
    lv = c.levels()
    assert np.array_equal(lv[-1], g["root"]) and np.array_equal(c.root(), g["root"])
    assert np.array_equal(level_dgs(lv, W), g["level_dg"])
    T = c.tensor()
    assert np.array_equal(dg(T), g["T_dg"])
    assert np.array_equal(T[g["ent_i"], g["ent_c"]], g["ent"])
    o = hb.brakedown_open(c, x, r, I)
    assert np.array_equal(dg(o["aggr_beta"]), g["aggr_beta_dg"]) and np.array_equal(dg(o["aggr_r"]), g["aggr_r_dg"])
    assert np.array_equal(dg(o["reply"]), g["reply_dg"])
    assert (o["paths"] == g["path"][None]).all()
    c.free()


@pytest.mark.gpu
def test_commit_without_quirk_builds_full_trees(hb, oracle):
    """left_left_quirk = 0: every column digest is the conventional Merkle root over its rows / 4 leaves, and so is the tree above them"""
    logn = 20
    c, poly, x, r, I = _commit(hb, oracle, logn, quirk=0)
    B, rows = shape(logn)
    T = c.tensor()
    lv = c.levels()
    sample = [0, 1, 5, B - 1, B, 2 * B - 1, 12345, 99999]
    for col in sample:
        h = oracle.blake3_64(np.ascontiguousarray(T[:, col]).view(np.uint8).reshape(-1, 64))
        while h.shape[0] > 1:
            h = oracle.blake3_64(h.reshape(-1, 64))
        assert np.array_equal(lv[col], h[0]), col
    top = hb.create_tree_blake(lv[:2 * B], quirk=0)
    assert np.array_equal(top, lv)
    c.free()


@pytest.mark.gpu
def test_commit_2e28_matches_reference(hb, oracle):
    """the reference's root, every level's digest and sampled columns at 2^28 (256 rows of B = 2^20)"""
    g = gold(28)
    B, rows = shape(28)
    hb.rng_reset()
    poly = hb.generate_randomness(1 << 28)            # test_PC's libc sequence: poly, then the graphs of n = B
    oracle.expander_init_store(B)
    hb.upload_graphs(B, graphs_from(oracle, B))
    c = hb.brakedown_commit(poly)
    del poly
    lv = c.levels()
    assert np.array_equal(lv[-1], g["root"])
    assert np.array_equal(level_dgs(lv, 2 * B), g["level_dg"])
    for k, col in enumerate(g["cols_idx"]):
        assert np.array_equal(c.tensor(int(col), 1)[:, 0], g["cols"][k]), int(col)
    c.free()


def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,timeout", [(20, 300), (28, 900)])
def test_host_test_pc_option3(logn, timeout):
    g = gold(logn)
    p = _test_pc([logn, 3, 128], timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    m = re.search(r"^root ([0-9a-f]{64})$", p.stdout, re.M)
    assert m and m.group(1) == bytes(g["root"]).hex(), p.stdout[-500:]
    assert re.search(r"^Commit time: \S+ seconds$", p.stdout, re.M) and re.search(r"^Total time: \S+ seconds$", p.stdout, re.M)
    m = re.search(r"^PC Open: pt = \S+, ps = (\S+) KB, vt = \S+ sec$", p.stdout, re.M)
    assert m, p.stdout[-500:]
    if "ps" in g:
        assert m.group(1) == "%f" % float(g["ps"][0])


def test_host_test_pc_other_baselines_still_refused():
    from __graft_entry__ import build_hip, build_host
    build_hip(); build_host()
    for opt in (2, 5, 6):
        p = _test_pc([20, opt, 128], 120)
        assert p.returncode == 255 and "comparison baseline" in p.stdout, (opt, p.returncode, p.stdout[-300:])


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [15, 30])
def test_commit_outside_range_is_einval(hb, logn):
    h = ctypes.c_void_p()
    rc = hb.lib.hobbit_brakedown_commit(hb.ctx, ctypes.c_void_p(0), ctypes.c_size_t(1 << logn), ctypes.c_int(1), ctypes.byref(h))
    assert rc == -2 and not h.value
