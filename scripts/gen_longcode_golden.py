"""scripts/gen_longcode_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref exists).

Fixtures of the long expander codes (tensor_row_size 8192 and 16384: codewords longer than one workgroup's LDS), recorded from the REAL
reference built into oracle/_ref.  New files only; the existing generators under oracle/ are imported, never changed.

  encode      tests/golden/longcode_encode.npz           encode_monolithic at n = 6000, 8192, 16384 on splitmix inputs, graphs from the
                                                         reference's own expander_init_store (libc sequence from the default seed)
  commit L K  tests/golden/longcode_root_2e<L>_K<K>.npz  test_PC(2^L, 4, K)'s commit_standard: root, sha256 of every Merkle level, sampled
                                                         leaves, tensor entries and paths (the shape of bigroot_2e28.npz)
  open L K    tests/golden/longcode_open_2e<L>_K<K>.json test_PC(2^L, 4, K)'s commit + open_standard under the mimc_hash recorder, up to the
                                                         first SHA3 call (oracle/gen_open_transcript.py's child mode)

One reference core: commit 2^28 K=16 ~11 min / ~28 GB, 2^26 ~2.5 min, 2^25 ~1 min.

usage: python scripts/gen_longcode_golden.py encode | commit 28 16 | commit 26 2 | commit 25 2 | open 25 2
"""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle  # noqa: E402
from oracle.pyoracle import splitmix_field  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ENCODE_SIZES = (6000, 8192, 16384)
NS = 64


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def encode_input(n):
    """the message every test encodes at size n"""
    return splitmix_field(n, 4000 + n)


def gen_encode():
    ref = pyoracle.Ref()
    out = {}
    for n in ENCODE_SIZES:
        ref.rng_reset()
        out["levels_%d" % n] = np.array([ref.expander_init_store(n)], np.int64)
        ref.encode_reset_scratch()
        d, ln = ref.encode_monolithic(encode_input(n))
        out["len_%d" % n] = np.array([ln], np.int64)
        out["code_%d" % n] = dg(d[:ln])
        idx = np.random.default_rng(n).integers(0, ln, NS)
        out["samp_idx_%d" % n] = idx
        out["samp_%d" % n] = d[idx].copy()
        print("encode n=%d: len %d" % (n, ln), flush=True)
    np.savez_compressed(os.path.join(GOLD, "longcode_encode.npz"), **out)


def sample_plan(logn, K):
    """deterministic sample positions shared with the tests (oracle/gen_big_roots.py's plan, any K)"""
    N = 1 << logn
    M = N // K
    trs = N // (K << 11)
    g = np.random.default_rng(2000 + 64 * logn + K)
    leaves = g.integers(0, M, NS)
    chunk = g.integers(0, K, NS); row = g.integers(0, 2 * trs, NS); col = g.integers(0, 4096, NS)
    row[:4] = [0, trs - 1, trs, 2 * trs - 1]
    q = [(0, 0), (5, 3), (4095, 2 * trs - 1), (100, trs), (2048, 7)]
    return M, trs, leaves, chunk, row, col, q


def gen_commit(logn, K):
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, "libhobbit_ref.so")
    shutil.copy(pyoracle.REF_SO, so)
    lib = pyoracle._dlopen_lazy(so)
    lib.ref_init()
    N = 1 << logn
    M, trs, leaves, chunk, row, col, q = sample_plan(logn, K)
    lv = np.zeros((2 * M, 32), np.uint8)
    t0 = time.time()
    lib.ref_test_pc_commit.restype = ctypes.c_size_t
    cnt = lib.ref_test_pc_commit(ctypes.c_size_t(N), ctypes.c_int(K), lv.ctypes.data_as(ctypes.c_void_p))
    dt = time.time() - t0
    assert cnt == 2 * M - 1
    out = {"root": lv[cnt - 1].copy(), "leaves_s": lv[leaves].copy(), "ref_seconds": np.array([dt]), "trs": np.array([trs], np.int64)}
    dgs, off, sz = [], 0, M
    while sz >= 1:
        dgs.append(dg(lv[off:off + sz])); off += sz; sz //= 2
    out["level_dg"] = np.stack(dgs)
    ts = np.zeros((NS, 2), np.uint64)
    for i in range(NS):
        r = np.array([row[i]], np.uint32); c = np.array([col[i]], np.uint32)
        lib.ref_tensor_get(ctypes.c_int(int(chunk[i])), r.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1),
                           ts[i:i + 1].ctypes.data_as(ctypes.c_void_p))
    out["tensor_s"] = ts
    depth = M.bit_length() - 1
    paths = np.zeros((len(q), depth, 32), np.uint8)
    for i, (c, r) in enumerate(q):
        d = lib.ref_open_tree_blake(ctypes.c_size_t(c), ctypes.c_size_t(r), ctypes.c_int(4096), paths[i].ctypes.data_as(ctypes.c_void_p))
        assert d == depth, (d, depth)
    out["paths"] = paths
    lib.ref_release_commit()
    np.savez_compressed(os.path.join(GOLD, "longcode_root_2e%d_K%d.npz" % (logn, K)), **out)
    print("2^%d K=%d (trs %d): reference commit_standard %.1f s, root %s" % (logn, K, trs, dt, lv[cnt - 1].tobytes().hex()), flush=True)
    shutil.rmtree(tmp)


def gen_open(logn, K):
    from ref_transcript import summarize
    script = os.path.join(ROOT, "oracle", "gen_open_transcript.py")
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "rec.bin")
        p = subprocess.run([sys.executable, script, "--child", str(logn), str(K)], capture_output=True, text=True, cwd=td,
                           env=dict(os.environ, HOBBIT_REC_STREAM=f), timeout=7200)
        rec = np.fromfile(f, np.uint64).reshape(-1, 6) if os.path.exists(f) else np.zeros((0, 6), np.uint64)
    d = summarize(rec)
    died = (p.stderr.strip().splitlines() or [""])[-1]
    assert "UNEXPECTED" not in p.stdout and p.returncode != 0 and "SHA3" in died, (p.returncode, p.stdout[-300:], p.stderr[-300:])
    d["died_with"] = died[died.rfind(".so: ") + 5:] if ".so: " in died else died[-160:]     # the loader's message without the library's path
    d["rc"] = p.returncode
    d["records"] = [[int(v) for v in r] for r in rec]
    d["source"] = ("scripts/gen_longcode_golden.py: the real reference's commit_standard + open_standard of test_PC(2^%d, 4, %d) under the mimc_hash "
                   "recorder (oracle/gen_open_transcript.py --child), up to the first SHA3 call" % (logn, K))
    name = "test_pc_2e%d_K%d" % (logn, K)
    json.dump({name: d}, open(os.path.join(GOLD, "longcode_open_2e%d_K%d.json" % (logn, K)), "w"), indent=None, separators=(",", ":"))
    print(name, d["count"], d["sha256"][:16], "|", d["died_with"][-60:], flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "encode":
        gen_encode()
    elif what == "commit":
        gen_commit(int(sys.argv[2]), int(sys.argv[3]))
    elif what == "open":
        gen_open(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(__doc__)
