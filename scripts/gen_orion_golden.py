"""scripts/gen_orion_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref exists).

Fixtures of the Orion comparison baseline, recorded from the REAL reference's own test_PC(2^n, 2, 128) (src/Our_PC.cpp:780-793).
scripts/orion_recorder.cpp (ours) is compiled into a temporary directory and loaded in front of the reference in a fresh child process,
behind oracle/_ref's libref_recorder_mimc.so (HOBBIT_REC_STREAM).  The reference is compiled for this into the same temporary directory by
oracle/Makefile's own recipe, with the two changes scripts/gen_brakingbase_golden.py documents (-ffp-contract=off; sumcheck.cpp unoptimised).
The graph dimensions of every B are asserted equal to those oracle/_ref's library draws.

The child runs under MALLOC_PERTURB_=255 (zero-filled allocations: open_parity_matrix reads past its lists, see scripts/gen_parity_golden.py)
and ends where the reference first needs SHA3 (not linked), inside the first _whir_prove of shockwave_prove(C_p): that death is expected and
asserted; the streamed files keep what ran before -- the commitment (the whole tensor and its tree), the column trees of C, C_p, C_w, and the
mimc transcript of prove_linear_code_batch, both multiplication trees, P2, P3, P4 and the two sumchecks of shockwave_prove(C_p).
shockwave_prove(C) and the Q^2 opening paths are never reached.  A second fresh child replays the libc draws (generate_randomness(N),
expander_init_store(B), generate_randomness(log2 N), generate_randomness(1), Q x (rand() % 2B, rand() % 2B)) through the reference's own
functions and gives x, I and J; that it stands on the recorded run's stream is checked through the polynomial (the tensor's message block).

  tests/golden/orion.npz   per shape, keys suffixed _<log2 N>: root, a digest of every level, sampled level-0 digests, the digest of the
                           whole tensor and sampled columns, x, I, J, the roots of C, C_p, C_w, P, the mimc transcript up to the first
                           SHA3 call, the reference's seconds

usage: python scripts/gen_orion_golden.py [logN ...]      (default: SHAPES)
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
SHAPES = (14, 16, 18, 20)                     # log2 N: B = 128, 256, 512, 1024
NS = 16
NCOLS = {14: 4, 16: 4, 18: 3, 20: 2}          # sampled columns (2B F each): the fixture stays within a few hundred KB
REFFLAGS = "-O3 -DNDEBUG -w -fPIC -march=x86-64-v3 -msha -mavx -ffp-contract=off -I$(REF)/src -idirafter /opt/conda/include"
RTLD_LAZY, RTLD_GLOBAL = 0x1, 0x100
MIMC = b"_Z9mimc_hashN5virgo12fieldElementES0_"
MT = b"_ZN11merkle_tree18merkle_tree_prover15MT_commit_BlakeEPN5virgo12fieldElementERSt6vectorIS4_I5_hashSaIS5_EESaIS7_EEi"
CT = b"_ZN11merkle_tree18merkle_tree_prover17create_tree_blakeEiRSt6vectorIS1_I5_hashSaIS2_EESaIS4_EEib"
OT = b"_ZN11merkle_tree18merkle_tree_prover15open_tree_blakeERSt6vectorIS1_I5_hashSaIS2_EESaIS4_EES1_ImSaImEEi"


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def sample_plan(logn):
    """deterministic sample positions shared with the tests"""
    N = 1 << logn; B = 1 << (logn // 2); S = 2 * B
    g = np.random.default_rng(7000 + logn)
    leaves = g.integers(0, N, NS); leaves[:3] = [0, 1, N - 1]
    cols = np.concatenate([[0, S - 1], g.integers(0, S, NS)])[:NCOLS[logn]]
    return dict(leaves=leaves, cols=cols)


def graph_dims(graph, n):
    out, dep, m = [], 0, n
    while m > 13:
        for kind in (0, 1):
            out.append(graph(dep, kind))
        m = int(0.211 * m); dep += 1
    return np.array(out, np.int64)


def child_record(logn):
    """fresh process: the real reference's test_PC(2^logn, 2, 128) with the recorders in front; does not return"""
    libc = ctypes.CDLL(None)
    libc.dlopen.restype = ctypes.c_void_p; libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libc.dlsym.restype = ctypes.c_void_p; libc.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    libc.dlerror.restype = ctypes.c_char_p
    h = []
    for k in ("HOBBIT_OR_MIMC_SO", "HOBBIT_OR_RECORDER", "HOBBIT_OR_REF_SO"):
        h.append(libc.dlopen(os.environ[k].encode(), RTLD_LAZY | RTLD_GLOBAL))
        assert h[-1], libc.dlerror()
    h_mimc, h_rec, h_ref = h
    assert libc.dlsym(None, MIMC) == libc.dlsym(h_mimc, MIMC) and libc.dlsym(h_ref, MIMC) != libc.dlsym(h_mimc, MIMC)
    for s in (MT, CT, OT):
        assert libc.dlsym(None, s) == libc.dlsym(h_rec, s) and libc.dlsym(h_ref, s) and libc.dlsym(h_ref, s) != libc.dlsym(h_rec, s), s
    fn = lambda hh, name, res, *args: ctypes.CFUNCTYPE(res, *args)(libc.dlsym(hh, name))  # noqa: E731
    fn(h_mimc, b"rec_set_next", None, ctypes.c_void_p)(libc.dlsym(h_ref, MIMC))
    fn(h_rec, b"or_set_next", None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)(libc.dlsym(h_ref, MT), libc.dlsym(h_ref, CT), libc.dlsym(h_ref, OT))
    fn(h_ref, b"ref_init", None)()
    fn(h_ref, b"ref_rng_reset", None)()                          # srandom(1): the state of a fresh process
    fn(h_mimc, b"rec_start", None)()
    fn(h_ref, b"_Z7test_PCmii", None, ctypes.c_size_t, ctypes.c_int, ctypes.c_int)(1 << logn, 2, 128)
    print("UNEXPECTED: test_PC returned", flush=True)
    os._exit(3)


def child_replay(logn, out_path, which):
    """fresh process: the same libc draws through the reference's own functions (which = temp: the library built here; ref: oracle/_ref's)"""
    if which == "temp":
        pyoracle.REF_SO = os.environ["HOBBIT_OR_REF_SO"]
    ref = pyoracle.Ref()
    N = 1 << logn; B = 1 << (logn // 2); Q = min(B, 4096)
    ref.rng_reset()
    poly = ref.generate_randomness(N)                  # test_PC (:758)
    total = ref.expander_init_store(B)                 # commit_standard_orion (:178)
    dims = graph_dims(lambda dep, kind: (lambda g: (g["L"], g["R"], g["degree"]))(ref.graph(dep, kind)), B)
    x = ref.generate_randomness(logn)                  # open_orion_standard's argument (:790)
    ref.generate_randomness(1)                         # r_v[0] (:540)
    libc = ctypes.CDLL(None)
    IJ = np.array([libc.rand() % (2 * B) for _ in range(2 * Q)], np.uint64)              # (:547-558) interleaved
    np.savez(out_path, x=x, I=IJ[0::2], J=IJ[1::2], poly_dg=dg(poly), dims=dims, total=np.array([total]))
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
        c0, c1, d = (int(v) for v in np.frombuffer(b[o:o + 24], np.uint64)); o += 24 + 32 * d
        out.append((c0, c1, d))
    return out


def gen(logn, env, td, res):
    N = 1 << logn; B = 1 << (logn // 2); S = 2 * B; Q = min(B, 4096)
    tag = "%d" % logn
    files = {k: os.path.join(td, "%s_%s.bin" % (k, tag)) for k in ("stream", "trees", "tensor", "commit", "paths")}
    e = dict(env, HOBBIT_REC_STREAM=files["stream"], HOBBIT_OR_TREES=files["trees"], HOBBIT_OR_TENSOR=files["tensor"], HOBBIT_OR_COMMIT=files["commit"],
             HOBBIT_OR_PATHS=files["paths"], MALLOC_PERTURB_="255")
    t0 = time.time()
    p = subprocess.run([sys.executable, __file__, "--child-record", str(logn)], capture_output=True, text=True, env=e, timeout=3600)
    dt = time.time() - t0
    assert p.returncode != 0 and "UNEXPECTED" not in p.stdout, (p.returncode, p.stdout[-400:])
    assert "SHA3" in p.stderr, "the child should end on the unlinked SHA3: " + p.stderr[-400:]
    assert "Commit time" in p.stdout, p.stdout[-400:]               # (recursive_prover_orion's own line dies in stdio's buffer)
    paths = read_paths(files["paths"])                               # the 240 column openings of shockwave_prove(C_p): none into the commitment
    assert all(c1 == 0 and d < logn for _, c1, d in paths), "the reference opened a commitment path before its first SHA3 call"
    rec = np.fromfile(files["stream"], np.uint64).reshape(-1, 6)
    lv = read_trees(files["commit"])
    assert len(lv) == 1 and lv[0].shape[0] == 2 * N - 1
    lv = lv[0]
    trees = read_trees(files["trees"])
    assert len(trees) >= 3 and trees[0].shape[0] == 2 * (Q * S // 16) - 1, [t.shape for t in trees]
    P = (trees[1].shape[0] + 1) // 2
    assert trees[2].shape[0] == 2 * (P // 4) - 1
    assert int(np.fromfile(files["tensor"], np.uint64, 1)[0]) == 4 * N
    T = np.fromfile(files["tensor"], np.uint64, offset=8).reshape(S, S, 2)
    rp = {}
    for which in ("temp", "ref"):
        f_rp = os.path.join(td, "rp_%s_%s.npz" % (tag, which))
        q = subprocess.run([sys.executable, __file__, "--child-replay", str(logn), f_rp, which], capture_output=True, text=True, env=env, timeout=3600)
        assert q.returncode == 0, (q.returncode, q.stderr[-800:])
        rp[which] = dict(np.load(f_rp))
    assert np.array_equal(rp["temp"]["dims"], rp["ref"]["dims"]) and rp["temp"]["total"][0] == rp["ref"]["total"][0], "graph dimensions differ from oracle/_ref's at B = %d" % B
    assert np.array_equal(rp["temp"]["I"], rp["ref"]["I"]) and np.array_equal(rp["temp"]["J"], rp["ref"]["J"])
    assert np.array_equal(dg(T[:B, :B].reshape(-1, 2)), rp["temp"]["poly_dg"]), "T[i][0..B) is row i of the replayed polynomial"
    sp = sample_plan(logn)
    dgs, off, sz = [], 0, N
    while sz >= 1:
        dgs.append(dg(lv[off:off + sz])); off += sz; sz //= 2
    k = "_" + tag
    res.update({"root" + k: lv[-1].copy(), "level_dg" + k: np.stack(dgs), "leaves_idx" + k: sp["leaves"], "leaves_s" + k: lv[sp["leaves"]].copy(), "T_dg" + k: dg(T),
                "cols_idx" + k: sp["cols"], "cols" + k: np.ascontiguousarray(T[:, sp["cols"]].transpose(1, 0, 2)), "I" + k: rp["temp"]["I"].astype(np.uint32),
                "J" + k: rp["temp"]["J"].astype(np.uint32), "x" + k: rp["temp"]["x"], "c_root" + k: trees[0][-1].copy(), "cp_root" + k: trees[1][-1].copy(),
                "cw_root" + k: trees[2][-1].copy(), "P" + k: np.array([P]), "transcript" + k: rec, "ref_seconds" + k: np.array([dt])})
    print("2^%d: B %d, Q %d, P %d, %d records before SHA3, root %s, child %.1f s" % (logn, B, Q, P, rec.shape[0], lv[-1].tobytes().hex()[:16], dt), flush=True)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-record":
        return child_record(int(a[1]))
    if a and a[0] == "--child-replay":
        return child_replay(int(a[1]), a[2], a[3])
    if not pyoracle.ref_available():
        sys.exit(__doc__)
    shapes = [int(s) for s in a] or list(SHAPES)
    td = tempfile.mkdtemp()
    try:
        out = os.path.join(td, "ref")
        mk = ["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "OUT=" + out]
        # sumcheck.cpp without optimisation first; the second call finds that object up to date and builds the rest
        subprocess.check_call(mk + ["REFFLAGS=" + REFFLAGS.replace("-O3", "-O0"), os.path.join(out, "obj", "sumcheck.o")])
        subprocess.check_call(mk + ["REFFLAGS=" + REFFLAGS, os.path.join(out, "libhobbit_ref.so")])
        rec_so = os.path.join(td, "liborion_recorder.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", rec_so, os.path.join(ROOT, "scripts", "orion_recorder.cpp")])
        env = dict(os.environ, HOBBIT_OR_MIMC_SO=os.path.join(ROOT, "oracle", "_ref", "libref_recorder_mimc.so"), HOBBIT_OR_RECORDER=rec_so,
                   HOBBIT_OR_REF_SO=os.path.join(out, "libhobbit_ref.so"))
        env.pop("MALLOC_PERTURB_", None)
        name = os.path.join(GOLD, "orion.npz")
        res = dict(np.load(name)) if a and os.path.exists(name) else {}
        for logn in shapes:
            gen(logn, env, td, res)
        res["shapes"] = np.array(sorted(int(key.split("_")[1]) for key in res if key.startswith("root_")))
        np.savez_compressed(name, **res)
        print("%s: %d bytes" % (name, os.path.getsize(name)))
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
