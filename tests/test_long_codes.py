"""Long expander codes: tensor_row_size 8192 and 16384, whose codewords (14 090 and 28 180 elements) do not fit in one workgroup's LDS.

Fixtures: scripts/gen_longcode_golden.py ran the REAL reference (oracle/_ref) once -- encode_monolithic at n = 6000 / 8192 / 16384, the
commitment of test_PC(2^28, 4, 16), (2^26, 4, 2) and (2^25, 4, 2), and the open transcript of test_PC(2^25, 4, 2) up to its first SHA3 call.
The CPU tests pin the oracle's restatement to those fixtures; the GPU tests hold the library to the fixtures and to the restatement."""
import hashlib
import json
import os
import sys
import numpy as np
import pytest
from golden_cases import dg
from oracle.pyoracle import splitmix_field

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gen_longcode_golden import ENCODE_SIZES, encode_input, sample_plan  # noqa: E402


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def level_digests(lv, M):
    off, sz, dgs = 0, M, []
    while sz >= 1:
        dgs.append(np.frombuffer(hashlib.sha256(lv[off:off + sz].tobytes()).digest(), np.uint8)); off += sz; sz //= 2
    return np.stack(dgs)


def graphs_from(oracle, n):
    lv, dep, m = {}, 0, n
    while m > 13:
        for kind in (0, 1):
            lv[(dep, kind)] = oracle.graph(dep, kind)
        m = int(0.211 * m); dep += 1
    return lv


def check_code(g, n, d):
    ln = int(g["len_%d" % n][0])
    assert np.array_equal(dg(d[:ln]), g["code_%d" % n]), n
    assert np.array_equal(d[g["samp_idx_%d" % n]], g["samp_%d" % n]), n
    return ln


# ---- CPU: the restatement the GPU open is compared against, pinned to the reference at the new sizes -----------------------------------
@pytest.mark.parametrize("n", ENCODE_SIZES)
def test_oracle_encode_long_vs_reference(oracle, n):
    g = gold("longcode_encode")
    oracle.rng_reset()
    assert oracle.expander_init_store(n) == int(g["levels_%d" % n][0])
    d, ln = oracle.encode_monolithic(encode_input(n))
    assert ln == int(g["len_%d" % n][0])
    check_code(g, n, d)
    assert not d[ln:].any()


@pytest.mark.parametrize("logN,K", [(25, 2), (26, 2)])
def test_oracle_commit_long_vs_reference(oracle, logN, K):
    """commit_standard at tensor_row_size 8192 (2^25) and 16384 (2^26) on test_PC's inputs: root and every Merkle level"""
    g = gold("longcode_root_2e%d_K%d" % (logN, K))
    N = 1 << logN
    M, trs, leaves, _, _, _, _ = sample_plan(logN, K)
    assert trs == int(g["trs"][0])
    oracle.rng_reset(); poly = oracle.generate_randomness(N); oracle.expander_init_store(trs)
    lv, _ = oracle.commit_standard(poly, K, trs, 1)
    assert np.array_equal(lv[-1], g["root"])
    assert np.array_equal(level_digests(lv, M), g["level_dg"])
    assert np.array_equal(lv[leaves], g["leaves_s"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ENCODE_SIZES)
@pytest.mark.parametrize("batch", [1, 5, 300])
def test_encode_long_vs_reference(hb, oracle, n, batch):
    """encode_monolithic past 160 KB of codeword (tiled outer steps + one-pass middle): column 0 is the fixture's message and must give the
    reference's codeword; the other columns are checked against the oracle (sampled) and by linearity.  In place (the commit's form, the
    codeword buffer holding garbage past the message) and out of place give the same columns, zeros past the codeword."""
    g = gold("longcode_encode")
    hb.rng_reset()
    assert hb.expander_init_store(n) == int(g["levels_%d" % n][0])
    x = splitmix_field(batch * n, 900 + n + batch).reshape(batch, n, 2)
    x[0] = encode_input(n)
    if batch >= 3:
        x[2] = hb.f_binop(0, x[0], x[1])
    out = hb.encode_monolithic(x)
    inp = hb.encode_monolithic(x, in_place=True)
    assert np.array_equal(out, inp)
    ln = check_code(g, n, out[0])
    assert not out[:, ln:].any()
    assert np.array_equal(out[:, :n], x)
    if batch >= 3:
        assert np.array_equal(out[2], hb.f_binop(0, out[0], out[1]))
    oracle.rng_reset(); oracle.expander_init_store(n)
    for b in sorted({batch // 2, batch - 1}):
        want, wl = oracle.encode_monolithic(x[b])
        assert wl == ln and np.array_equal(out[b], want), b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6000, 8192])
def test_encode_long_full_range_weights_vs_oracle(hb, oracle, n):
    """graphs with full-range F_{p^2} weights on every level (the general-weight kernels), against the oracle with the same weights"""
    oracle.rng_reset(); oracle.expander_init_store(n)
    lv = graphs_from(oracle, n)
    for i, key in enumerate(sorted(lv)):
        w = splitmix_field(lv[key]["L"] * lv[key]["degree"], 300 + i)
        lv[key]["w"] = w
        oracle.graph_set_weights(key[0], key[1], w)
    hb.upload_graphs(n, lv)
    x = splitmix_field(3 * n, 17 + n).reshape(3, n, 2)
    got = hb.encode_monolithic(x)
    assert np.array_equal(got, hb.encode_monolithic(x, in_place=True))
    for b in range(3):
        want, ln = oracle.encode_monolithic(x[b])
        assert np.array_equal(got[b], want), b


@pytest.mark.gpu
@pytest.mark.parametrize("logN,K", [(28, 16), (26, 2), (25, 2)])
def test_commit_standard_long_vs_reference(hb, logN, K):
    """commit_standard on test_PC(2^logN, 4, K)'s inputs at tensor_row_size 8192 / 16384 against the REAL reference's commitment:
    root, sha256 of every Merkle level, sampled leaves, tensor entries (rows past the codeword included) and open_tree_blake paths"""
    g = gold("longcode_root_2e%d_K%d" % (logN, K))
    N = 1 << logN
    M, trs, leaves, chunk, row, col, qs = sample_plan(logN, K)
    hb.rng_reset()
    poly = hb.generate_randomness(N)
    hb.expander_init_store(trs)
    d = hb.to_device(poly); del poly
    c = hb.commit_standard((d, N), K, trs, 1)
    assert np.array_equal(c.root(), g["root"])
    lv = c.levels()
    assert np.array_equal(level_digests(lv, M), g["level_dg"])
    assert np.array_equal(lv[leaves], g["leaves_s"])
    del lv
    for i in range(len(chunk)):
        assert np.array_equal(c.gather([row[i]], [col[i]])[0, chunk[i]], g["tensor_s"][i]), i
    for i, (cc, rr) in enumerate(qs):
        assert np.array_equal(c.open_tree_blake(cc, rr), g["paths"][i]), i
    c.free(); d.free()


SP_KEYS = ("I", "q1", "r1", "vr1", "fin1", "q2", "r2", "vr2", "fin2", "iters", "wq", "wa", "wroots", "wscal", "wchecks", "whir_root",
           "reply", "paths", "qn", "qidx", "qreply", "qpaths", "final_pb")


@pytest.mark.gpu
@pytest.mark.parametrize("logN,K", [(25, 2), (26, 2)])
def test_open_standard_long_vs_oracle(hb, oracle, logN, K):
    """open_standard with the linear-time code at tensor_row_size 8192 / 16384 (prove_linear_code / evaluate_parity_matrix at n = trs, the
    tensor code of the aggregate through the long encode): every transcript bit-exact against the oracle, both exit(-1) checks hold"""
    import ctypes
    libc = ctypes.CDLL(None)
    N = 1 << logN; trs = N // (K << 11)
    oracle.rng_reset(); poly = oracle.generate_randomness(N); oracle.expander_init_store(trs)
    x = oracle.generate_randomness(logN)
    queries = 5900
    libc.srandom(777); want = oracle.open_standard(poly, K, trs, x, queries)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    c = hb.commit_standard(poly, K, trs, 1)
    libc.srandom(777); got = hb.open_standard(poly, c, x, queries, want_paths=False)
    c.free()
    assert want["checks"].tolist() == [1, 1, 1] and got["checks"].tolist() == [1, 1, 1]
    for k in ("I", "scalars", "poly", "r", "vr", "fin", "roots"):
        assert np.array_equal(got[k], want[k]), k
    for sp in ("sp_c", "sp_f"):
        has_whir = int(want[sp]["iters"][0]) > 0
        assert want[sp]["wchecks"].tolist() == ([1, 1] if has_whir else [0, 0]), sp
        for k in SP_KEYS:
            assert np.array_equal(got[sp][k], want[sp][k]), (sp, k)


@pytest.mark.gpu
def test_open_standard_long_transcript_vs_reference(hb, monkeypatch):
    """the library's own transcript of test_PC(2^25, 4, 2) (tensor_row_size 8192) against the REAL reference's, record for record up to the
    reference's first SHA3 call (the reference runs shockwave_prove(C_c) before P5, the library on one thread after it)"""
    logn, K = 25, 2
    fix = json.load(open(os.path.join(GOLD, "longcode_open_2e%d_K%d.json" % (logn, K))))["test_pc_2e%d_K%d" % (logn, K)]
    ref = np.array(fix["records"], np.uint64).reshape(-1, 6)
    assert ref.shape[0] == fix["count"] > 200
    monkeypatch.setenv("HOBBIT_OPEN_THREADS", "0")
    N = 1 << logn; trs = N // (K << 11)
    hb.rng_reset()
    poly = hb.generate_randomness(N)
    hb.expander_init_store(trs)
    c = hb.commit_standard(poly, K, trs, 1)
    x = hb.generate_randomness(logn)
    hb.lib.hobbit_transcript_record(1)
    res = hb.open_standard(poly, c, x, 5900, want_paths=False)
    hb.lib.hobbit_transcript_record(0)
    n = hb.lib.hobbit_transcript_count()
    mine = np.zeros((n, 6), np.uint64)
    hb.lib.hobbit_transcript_read(mine.ctypes.data, n)
    c.free()
    assert res["checks"].tolist() == [1, 1, 1]
    cols = 2 * (N // K) // trs
    R1 = (2 * trs).bit_length() - 1; logc = cols.bit_length() - 1; R3 = R1 + logc
    head = 3 * (R1 + logc + 2 * R3) + 2 * 4
    assert np.array_equal(mine[:head], ref[:head]), "P1..P4 differ from the reference at record %d" % int(np.nonzero((mine[:head] != ref[:head]).any(axis=1))[0][0])
    rest = ref[head:]
    hits = [j for j in range(head, n - len(rest) + 1) if np.array_equal(mine[j], rest[0])]
    assert hits, "the reference's shockwave_prove(C_c) transcript does not start anywhere in the library's"
    j0 = hits[0]
    assert np.array_equal(mine[j0:j0 + len(rest)], rest)
    assert j0 - head == 3 * logc + 2


@pytest.mark.gpu
def test_test_pc_driver_2e28_K16():
    """`./pigeon 28 4 16` over the host mirror (tensor_row_size 8192): exits 0, prints >>OK and the reference's commitment root"""
    import subprocess
    from __graft_entry__ import PKG, build_host
    build_host()
    r = subprocess.run([os.path.join(PKG, "host", "test_pc"), "28", "4", "16"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert ">>OK" in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("root ")]
    assert line and line[0].split()[1] == gold("longcode_root_2e28_K16")["root"].tobytes().hex(), line
