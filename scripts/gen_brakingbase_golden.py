"""scripts/gen_brakingbase_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref exists).

Fixtures of the Braking base comparison baseline, recorded from the REAL reference's own test_PC(N, 5, K) (src/Our_PC.cpp:827-842).
scripts/brakingbase_recorder.cpp (ours) is compiled into a temporary directory and loaded in front of the reference in a fresh child process,
behind oracle/_ref's libref_recorder_mimc.so (HOBBIT_REC_STREAM).  The reference is compiled for this into the same temporary directory by
oracle/Makefile's own recipe, with the two changes the other generators document: -ffp-contract=off (scripts/gen_brakedown_golden.py: the
reference's own build passes no -O flag, and a contracted n * (r - 1) - L changes a graph size at n = 2^20) and sumcheck.cpp unoptimised
(scripts/gen_parity_golden.py: generate_read_transcript runs off its end at -O3).  The graph dimensions of every trs are asserted equal to those
oracle/_ref's library draws.

The child runs under MALLOC_PERTURB_=255 (zero-filled allocations: open_parity_matrix reads past its lists, see scripts/gen_parity_golden.py)
and ends where the reference first needs SHA3 (not linked), inside the first _whir_prove of shockwave_prove(C_p): that death is expected and
asserted; the streamed files keep what ran before -- the commitment, C_c, C_p, C_w, the 2935 queries with their paths, and the mimc transcript
of prove_linear_code, both multiplication trees, P2, P3, P4 and the two sumchecks of shockwave_prove(C_p).  shockwave_prove(C_c) is never reached.
A second fresh child replays the libc draws (generate_randomness(N), expander_init_store(trs), generate_randomness(log2 N),
generate_randomness(1), 2935 x rand() % 2 trs) through the reference's own functions: its I must equal the recorded one.

  tests/golden/brakingbase.npz   per shape (N, K), keys suffixed _<log2 N>_<K>: root, a digest of every level, sampled level-0 digests, the
                                 digest of the whole encoded matrix and sampled columns, I, the opening path, x, the roots of C_c, C_p, C_w,
                                 the mimc transcript up to the first SHA3 call, the reference's seconds

usage: python scripts/gen_brakingbase_golden.py [logN:K ...]      (default: SHAPES)
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("REF", "/root/reference")
SHAPES = ((13, 64), (14, 128), (16, 64), (19, 128), (16, 8))          # (log2 N, K): trs 128, 128, 1024, 4096, 8192
QUERIES = 2935
NS = 16
REFFLAGS = "-O3 -DNDEBUG -w -fPIC -march=x86-64-v3 -msha -mavx -ffp-contract=off -I$(REF)/src -idirafter /opt/conda/include"
RTLD_LAZY, RTLD_GLOBAL = 0x1, 0x100
MIMC = b"_Z9mimc_hashN5virgo12fieldElementES0_"
MT = b"_ZN11merkle_tree18merkle_tree_prover15MT_commit_BlakeEPN5virgo12fieldElementERSt6vectorIS4_I5_hashSaIS5_EESaIS7_EEi"
CT = b"_ZN11merkle_tree18merkle_tree_prover17create_tree_blakeEiRSt6vectorIS1_I5_hashSaIS2_EESaIS4_EEib"
OT = b"_ZN11merkle_tree18merkle_tree_prover15open_tree_blakeERSt6vectorIS1_I5_hashSaIS2_EESaIS4_EES1_ImSaImEEi"


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def sample_plan(logn, K):
    """deterministic sample positions shared with the tests"""
    trs = (1 << logn) // K; W = 2 * trs
    g = np.random.default_rng(9000 + 64 * logn + K)
    leaves = g.integers(0, W, NS); leaves[:3] = [0, 1, W - 1]
    cols = np.concatenate([[0, 1, trs - 1, trs, W - 1], g.integers(0, W, NS - 5)])
    return dict(leaves=leaves, cols=cols)


def graph_dims(graph, n):
    out, dep, m = [], 0, n
    while m > 13:
        for kind in (0, 1):
            out.append(graph(dep, kind))
        m = int(0.211 * m); dep += 1
    return np.array(out, np.int64)


def child_record(logn, K):
    """fresh process: the real reference's test_PC(2^logn, 5, K) with the recorders in front; does not return"""
    libc = ctypes.CDLL(None)
    libc.dlopen.restype = ctypes.c_void_p; libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libc.dlsym.restype = ctypes.c_void_p; libc.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    libc.dlerror.restype = ctypes.c_char_p
    h = []
    for k in ("HOBBIT_BB_MIMC_SO", "HOBBIT_BB_RECORDER", "HOBBIT_BB_REF_SO"):
        h.append(libc.dlopen(os.environ[k].encode(), RTLD_LAZY | RTLD_GLOBAL))
        assert h[-1], libc.dlerror()
    h_mimc, h_rec, h_ref = h
    assert libc.dlsym(None, MIMC) == libc.dlsym(h_mimc, MIMC) and libc.dlsym(h_ref, MIMC) != libc.dlsym(h_mimc, MIMC)
    for s in (MT, CT, OT):
        assert libc.dlsym(None, s) == libc.dlsym(h_rec, s) and libc.dlsym(h_ref, s) and libc.dlsym(h_ref, s) != libc.dlsym(h_rec, s), s
    fn = lambda hh, name, res, *args: ctypes.CFUNCTYPE(res, *args)(libc.dlsym(hh, name))  # noqa: E731
    fn(h_mimc, b"rec_set_next", None, ctypes.c_void_p)(libc.dlsym(h_ref, MIMC))
    fn(h_rec, b"bb_set_next", None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)(libc.dlsym(h_ref, MT), libc.dlsym(h_ref, CT), libc.dlsym(h_ref, OT))
    fn(h_ref, b"ref_init", None)()
    fn(h_ref, b"ref_rng_reset", None)()                          # srandom(1): the state of a fresh process
    fn(h_mimc, b"rec_start", None)()
    fn(h_ref, b"_Z7test_PCmii", None, ctypes.c_size_t, ctypes.c_int, ctypes.c_int)(1 << logn, 5, K)
    print("UNEXPECTED: test_PC returned", flush=True)
    os._exit(3)


def child_replay(logn, K, out_path, which):
    """fresh process: the same libc draws through the reference's own functions (which = temp: the library built here; ref: oracle/_ref's)"""
    if which == "temp":
        pyoracle.REF_SO = os.environ["HOBBIT_BB_REF_SO"]
    ref = pyoracle.Ref()
    N = 1 << logn; trs = N // K
    ref.rng_reset()
    poly = ref.generate_randomness(N)                  # test_PC (:758)
    total = ref.expander_init_store(trs)               # (:829)
    dims = graph_dims(lambda dep, kind: (lambda g: (g["L"], g["R"], g["degree"]))(ref.graph(dep, kind)), trs)
    x = ref.generate_randomness(logn)                  # open_brakingbase's argument (:838)
    ref.generate_randomness(1)                         # r_v[0] (:374)
    libc = ctypes.CDLL(None)
    I = np.array([libc.rand() % (2 * trs) for _ in range(QUERIES)], np.uint64)          # (:382-385)
    np.savez(out_path, x=x, I=I, poly_dg=dg(poly), dims=dims, total=np.array([total]))
    os._exit(0)


def read_trees(path):
    out = []
    b = open(path, "rb").read(); o = 0
    while o < len(b):
        n = int(np.frombuffer(b[o:o + 8], np.uint64)[0]); o += 8
        out.append(np.frombuffer(b[o:o + 32 * (2 * n - 1)], np.uint8).reshape(2 * n - 1, 32).copy()); o += 32 * (2 * n - 1)
    return out


def read_paths(path):
    out = []
    b = open(path, "rb").read(); o = 0
    while o < len(b):
        c0, c1, d = (int(v) for v in np.frombuffer(b[o:o + 24], np.uint64)); o += 24
        out.append((c0, c1, np.frombuffer(b[o:o + 32 * d], np.uint8).reshape(d, 32).copy())); o += 32 * d
    return out


def gen(logn, K, env, td, res):
    N = 1 << logn; trs = N // K; W = 2 * trs
    tag = "%d_%d" % (logn, K)
    files = {k: os.path.join(td, "%s_%s.bin" % (k, tag)) for k in ("stream", "trees", "tensor", "paths")}
    e = dict(env, HOBBIT_REC_STREAM=files["stream"], HOBBIT_BB_TREES=files["trees"], HOBBIT_BB_TENSOR=files["tensor"], HOBBIT_BB_PATHS=files["paths"], MALLOC_PERTURB_="255")
    t0 = time.time()
    p = subprocess.run([sys.executable, __file__, "--child-record", str(logn), str(K)], capture_output=True, text=True, env=e, timeout=3600)
    dt = time.time() - t0
    assert p.returncode != 0 and "UNEXPECTED" not in p.stdout, (p.returncode, p.stdout[-400:])
    assert "SHA3" in p.stderr, "the child should end on the unlinked SHA3: " + p.stderr[-400:]
    assert "%d,%d" % (trs, K) in p.stdout, p.stdout[-400:]          # commit_brakingbase's own line (:119)
    rec = np.fromfile(files["stream"], np.uint64).reshape(-1, 6)
    trees = read_trees(files["trees"])
    assert len(trees) >= 4 and [t.shape[0] for t in trees[:2]] == [2 * W - 1, 2 * (trs // 8) - 1], [t.shape for t in trees]
    P = (trees[2].shape[0] + 1) // 2
    assert trees[3].shape[0] == 2 * (P // 4) - 1
    hd = np.fromfile(files["tensor"], np.uint64, 2)
    assert (int(hd[0]), int(hd[1])) == (K, W)
    T = np.fromfile(files["tensor"], np.uint64, offset=16).reshape(K, W, 2)
    paths = read_paths(files["paths"])
    assert len(paths) >= QUERIES and all(c0 == 0 and len(pt) == W.bit_length() - 1 for c0, _, pt in paths[:QUERIES])
    I = np.array([c1 for _, c1, _ in paths[:QUERIES]], np.uint64)
    assert all(np.array_equal(pt, paths[0][2]) for _, _, pt in paths[:QUERIES]), "every opening path should be leaf 0's"
    rp = {}
    for which in ("temp", "ref"):
        f_rp = os.path.join(td, "rp_%s_%s.npz" % (tag, which))
        q = subprocess.run([sys.executable, __file__, "--child-replay", str(logn), str(K), f_rp, which], capture_output=True, text=True, env=env, timeout=3600)
        assert q.returncode == 0, (q.returncode, q.stderr[-800:])
        rp[which] = dict(np.load(f_rp))
    assert np.array_equal(rp["temp"]["dims"], rp["ref"]["dims"]) and rp["temp"]["total"][0] == rp["ref"]["total"][0], "graph dimensions differ from oracle/_ref's at trs = %d" % trs
    assert np.array_equal(rp["temp"]["I"], I), "the replayed draws do not give the recorded queries"
    assert np.array_equal(dg(T[:, :trs].reshape(-1, 2)), rp["temp"]["poly_dg"]), "tensor[0][i][0..trs) is row i of the replayed polynomial"
    lv = trees[0]; sp = sample_plan(logn, K)
    dgs, off, sz = [], 0, W
    while sz >= 1:
        dgs.append(dg(lv[off:off + sz])); off += sz; sz //= 2
    k = "_" + tag
    res.update({"root" + k: lv[-1].copy(), "level_dg" + k: np.stack(dgs), "leaves_idx" + k: sp["leaves"], "leaves_s" + k: lv[sp["leaves"]].copy(), "T_dg" + k: dg(T),
                "cols_idx" + k: sp["cols"], "cols" + k: np.ascontiguousarray(T[:, sp["cols"]].transpose(1, 0, 2)), "I" + k: I.astype(np.uint32), "path" + k: paths[0][2],
                "x" + k: rp["temp"]["x"], "cc_root" + k: trees[1][-1].copy(), "cp_root" + k: trees[2][-1].copy(), "cw_root" + k: trees[3][-1].copy(), "P" + k: np.array([P]),
                "transcript" + k: rec, "ref_seconds" + k: np.array([dt])})
    print("(2^%d, %d): trs %d, P %d, %d records before SHA3, root %s, child %.1f s" % (logn, K, trs, P, rec.shape[0], lv[-1].tobytes().hex()[:16], dt), flush=True)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-record":
        return child_record(int(a[1]), int(a[2]))
    if a and a[0] == "--child-replay":
        return child_replay(int(a[1]), int(a[2]), a[3], a[4])
    if not pyoracle.ref_available():
        sys.exit(__doc__)
    shapes = [tuple(int(v) for v in s.split(":")) for s in a] or list(SHAPES)
    td = tempfile.mkdtemp()
    try:
        out = os.path.join(td, "ref")
        mk = ["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "OUT=" + out]
        # sumcheck.cpp without optimisation first; the second call finds that object up to date and builds the rest
        subprocess.check_call(mk + ["REFFLAGS=" + REFFLAGS.replace("-O3", "-O0"), os.path.join(out, "obj", "sumcheck.o")])
        subprocess.check_call(mk + ["REFFLAGS=" + REFFLAGS, os.path.join(out, "libhobbit_ref.so")])
        rec_so = os.path.join(td, "libbrakingbase_recorder.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", rec_so, os.path.join(ROOT, "scripts", "brakingbase_recorder.cpp"), "-ldl"])
        env = dict(os.environ, HOBBIT_BB_MIMC_SO=os.path.join(ROOT, "oracle", "_ref", "libref_recorder_mimc.so"), HOBBIT_BB_RECORDER=rec_so,
                   HOBBIT_BB_REF_SO=os.path.join(out, "libhobbit_ref.so"))
        env.pop("MALLOC_PERTURB_", None)
        name = os.path.join(GOLD, "brakingbase.npz")
        res = dict(np.load(name)) if a and os.path.exists(name) else {}
        for logn, K in shapes:
            gen(logn, K, env, td, res)
        done = sorted({tuple(int(v) for v in key.split("_")[1:]) for key in res if key.startswith("root_")})
        res["shapes"] = np.array(done)
        np.savez_compressed(name, **res)
        print("%s: %d bytes" % (name, os.path.getsize(name)))
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
