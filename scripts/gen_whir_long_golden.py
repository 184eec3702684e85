#!/usr/bin/env python3
"""Record tests/golden/whir_long.npz: whir_commit + _whir_prove at N = 2^25 and 2^26 from the oracle (oracle/hobbit_oracle.c, CPU only).

The oracle takes minutes at these sizes (one core), too long for a test, so tests/test_whir_long.py compares hobbit_whir_prove_any with this
recording.  Inputs: poly = splitmix_field(N, SEED_POLY + logN), x = splitmix_field(logN, SEED_X + logN), srandom(7) in front of the proof.
Stored per size (key prefix "<logN>_"): iters, poly, a, roots, scal, checks, qn, qidx, final_pb in full; the whir_commit root; rand() after
the call; SHA-256 of qreply and of qpaths; and the first path of every query round (for diagnosis when a digest differs).

    python scripts/gen_whir_long_golden.py [logN ...]        (default: 25 26; sizes already in the file are kept)
"""
import ctypes
import hashlib
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle                                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "whir_long.npz")
SEED_POLY, SEED_X, SRANDOM = 9100, 9200, 7


def first_paths(res, N):
    """the first Merkle path of every query round, concatenated (round t reads the layer of (2N) >> t elements: depth log2 of a quarter of it)"""
    out, off = [], 0
    for t, n in enumerate(res["qn"]):
        depth = ((2 * N) >> t).bit_length() - 1 - 2
        if n:
            out.append(res["qpaths"][off:off + 32 * depth])
        off += int(n) * 32 * depth
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def record(orc, logN):
    libc = ctypes.CDLL(None)
    N = 1 << logN
    p = pyoracle.splitmix_field(N, SEED_POLY + logN); x = pyoracle.splitmix_field(logN, SEED_X + logN)
    t0 = time.time(); com, lv = orc.whir_commit(p); t1 = time.time()
    libc.srandom(SRANDOM); res = orc.whir_prove(p, x, com, lv); after = libc.rand(); t2 = time.time()
    print("logN=%d: commit %.1f s, proof %.1f s, iters %d, queries %s" % (logN, t1 - t0, t2 - t1, int(res["iters"][0]), res["qn"].tolist()), flush=True)
    assert res["checks"].tolist() == [1, 1]
    g = {k: res[k] for k in ("iters", "poly", "a", "roots", "scal", "checks", "qn", "qidx", "final_pb")}
    g["commit_root"] = np.frombuffer(bytes(lv[-1]), np.uint8).copy()
    g["rand_after"] = np.array([after], np.int64)
    g["qreply_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(res["qreply"]).tobytes()).digest(), np.uint8).copy()
    g["qpaths_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(res["qpaths"]).tobytes()).digest(), np.uint8).copy()
    g["first_paths"] = first_paths(res, N)
    return {"%d_%s" % (logN, k): v for k, v in g.items()}


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [25, 26]
    orc = pyoracle.Oracle()
    data = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for logN in sizes:
        data.update(record(orc, logN))
        np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
