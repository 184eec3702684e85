"""scripts/gen_parity_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref exists).

Fixtures of the parity-matrix family -- commit_parity_matrix, open_parity_matrix, prove_linear_code_batch (src/sumcheck.cpp:2671-2885,
3201-3221) -- recorded from the REAL reference.  scripts/parity_recorder.cpp (ours) is compiled into a temporary directory and loaded in front
of the reference in fresh child processes, behind oracle/_ref's libref_recorder_mimc.so (HOBBIT_REC_STREAM).  The reference is compiled for
this into the same temporary directory by oracle/Makefile's own recipe, with sumcheck.cpp UNOPTIMISED (a REFFLAGS override for that one
object): generate_read_transcript (:2600-2620) is declared int and returns nothing, and the -O3 build runs off its end inside
open_parity_matrix (the hazard oracle/Makefile documents for read_memory_circuit).  The graph dimensions of every n are asserted equal to
those oracle/_ref's library draws.

open_parity_matrix reads access_idx1[i] / access_idx2[i] for m <= i < P past the vectors' size (:2756-2763): its transcript depends on what
the allocator left there.  Every case runs in a fresh child under MALLOC_PERTURB_=255 -- a glibc tunable that makes malloc hand out zero-filled
memory -- which is the defined result (index padding = 0); one more child with another fill byte records that the transcripts differ.
The run ends where the reference first needs SHA3 (not linked), inside the first _whir_prove of shockwave_prove(C_p); the streamed files keep
what ran before.

  tests/golden/parity_matrix.npz   n = 128, 1024, 4096: m, P, digests of the three lists, C_p's root and a digest of each tree level, r1, r2,
                                   the mimc transcript up to the first SHA3 call, C_w's root, the reference's seconds;
                                   (n, count) = (128, 2), (128, 64), (4096, 4): the whole batch proof, its challenges, a digest of the codewords

usage: python scripts/gen_parity_golden.py
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
NS = (128, 1024, 4096)
BATCHES = ((128, 2), (128, 64), (4096, 4))
REFFLAGS = "-O3 -DNDEBUG -w -fPIC -march=x86-64-v3 -msha -mavx -I%s/src -idirafter /opt/conda/include" % REF
RTLD_LAZY, RTLD_GLOBAL = 0x1, 0x100
MIMC = b"_Z9mimc_hashN5virgo12fieldElementES0_"
MT = b"_ZN11merkle_tree18merkle_tree_prover15MT_commit_BlakeEPN5virgo12fieldElementERSt6vectorIS4_I5_hashSaIS5_EESaIS7_EEi"
CT = b"_ZN11merkle_tree18merkle_tree_prover17create_tree_blakeEiRSt6vectorIS1_I5_hashSaIS2_EESaIS4_EEib"
P_ = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def _load():
    """mimc recorder, parity recorder, reference: in that order, all global, lazily bound"""
    libc = ctypes.CDLL(None)
    libc.dlopen.restype = ctypes.c_void_p; libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libc.dlsym.restype = ctypes.c_void_p; libc.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    libc.dlerror.restype = ctypes.c_char_p
    h = {}
    for k in ("HOBBIT_PM_MIMC_SO", "HOBBIT_PM_RECORDER", "HOBBIT_PM_REF_SO"):
        h[k] = libc.dlopen(os.environ[k].encode(), RTLD_LAZY | RTLD_GLOBAL)
        assert h[k], libc.dlerror()
    h_mimc, h_rec, h_ref = h["HOBBIT_PM_MIMC_SO"], h["HOBBIT_PM_RECORDER"], h["HOBBIT_PM_REF_SO"]
    assert libc.dlsym(None, MIMC) == libc.dlsym(h_mimc, MIMC) and libc.dlsym(h_ref, MIMC) != libc.dlsym(h_mimc, MIMC)
    for s in (MT, CT):
        assert libc.dlsym(None, s) == libc.dlsym(h_rec, s) and libc.dlsym(h_ref, s) and libc.dlsym(h_ref, s) != libc.dlsym(h_rec, s), s
    fn = lambda hh, name, res, *args: ctypes.CFUNCTYPE(res, *args)(libc.dlsym(hh, name))  # noqa: E731
    fn(h_mimc, b"rec_set_next", None, ctypes.c_void_p)(libc.dlsym(h_ref, MIMC))
    fn(h_rec, b"pr_set_next", None, ctypes.c_void_p, ctypes.c_void_p)(libc.dlsym(h_ref, MT), libc.dlsym(h_ref, CT))
    fn(h_ref, b"ref_init", None)()
    fn(h_ref, b"ref_rng_reset", None)()                          # srandom(1): the state of a fresh process
    return libc, h_mimc, h_rec, h_ref, fn


def _dims(fn, h_ref, n):
    out = []
    gd = fn(h_ref, b"ref_graph_dims", ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
    dep, m = 0, n
    while m > 13:
        for kind in (0, 1):
            R = ctypes.c_longlong(); d = ctypes.c_int()
            L = gd(dep, kind, ctypes.addressof(R), ctypes.addressof(d))
            out.append((L, R.value, d.value))
        m = int(0.211 * m); dep += 1
    return np.array(out, np.int64)


def child_lists(n, out_path):
    """fresh process: the graphs, their dimensions and the three lists; returns normally"""
    libc, h_mimc, h_rec, h_ref, fn = _load()
    total = fn(h_rec, b"pr_graphs", ctypes.c_longlong, ctypes.c_int)(n)
    lists = fn(h_rec, b"pr_lists", ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
    m = lists(n, None, None, None)
    i1 = np.zeros(m, np.int32); i2 = np.zeros(m, np.int32); w = np.zeros((m, 2), np.uint64)
    assert lists(n, P_(i1), P_(i2), P_(w)) == m
    np.savez(out_path, dims=_dims(fn, h_ref, n), total=np.array([total]), m=np.array([m]), idx1_dg=dg(i1.astype(np.uint32)), idx2_dg=dg(i2.astype(np.uint32)), weight_dg=dg(w))
    os._exit(0)


def child_dims(n, out_path):
    """fresh process: the graph dimensions oracle/_ref's own library draws"""
    ref = pyoracle.Ref()
    ref.rng_reset(); total = ref.expander_init_store(n)
    out = []
    dep, m = 0, n
    while m > 13:
        for kind in (0, 1):
            g = ref.graph(dep, kind); out.append((g["L"], g["R"], g["degree"]))
        m = int(0.211 * m); dep += 1
    np.savez(out_path, dims=np.array(out, np.int64), total=np.array([total]))
    os._exit(0)


def child_open(n, out_path):
    """fresh process: graphs, commit_parity_matrix, r1, r2, open_parity_matrix -- which ends at the first SHA3 call; everything is streamed to files"""
    libc, h_mimc, h_rec, h_ref, fn = _load()
    fn(h_rec, b"pr_graphs", ctypes.c_longlong, ctypes.c_int)(n)
    t0 = time.time()
    fn(h_rec, b"pr_commit", None, ctypes.c_int)(n)
    np.save(out_path, np.array([time.time() - t0]))
    fn(h_mimc, b"rec_start", None)()
    r12 = np.zeros((64, 2), np.uint64)
    fn(h_rec, b"pr_open", None, ctypes.c_int, ctypes.c_void_p)(n, P_(r12))
    print("UNEXPECTED: open_parity_matrix returned", flush=True)
    os._exit(3)


def child_batch(n, count, out_path):
    libc, h_mimc, h_rec, h_ref, fn = _load()
    fn(h_rec, b"pr_graphs", ctypes.c_longlong, ctypes.c_int)(n)
    l = (2 * n).bit_length() - 1; lc = count.bit_length() - 1
    cw = np.zeros((count, 2 * n, 2), np.uint64); q = np.zeros((l, 3, 2), np.uint64); r = np.zeros((l, 2), np.uint64); vr = np.zeros((2, 2), np.uint64)
    fin = np.zeros(2, np.uint64); r1 = np.zeros((l, 2), np.uint64); r2 = np.zeros((lc, 2), np.uint64)
    t0 = time.time()
    rounds = fn(h_rec, b"pr_batch", ctypes.c_int, ctypes.c_int, ctypes.c_int, *([ctypes.c_void_p] * 7))(n, count, P_(cw), P_(q), P_(r), P_(vr), P_(fin), P_(r1), P_(r2))
    assert rounds == l
    np.savez(out_path, cw_dg=dg(cw), cw_s=cw[:, :8].copy(), poly=q, r=r, vr=vr, fin=fin, r1=r1, r2=r2, ref_seconds=np.array([time.time() - t0]))
    os._exit(0)


def run_child(args, env, perturb=None, may_die=False):
    e = dict(env)
    if perturb is not None:
        e["MALLOC_PERTURB_"] = str(perturb)
    p = subprocess.run([sys.executable, __file__] + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=4 * 3600)
    assert may_die or p.returncode == 0, (args, p.returncode, p.stdout[-400:], p.stderr[-800:])
    return p


def read_trees(path):
    out = []
    b = open(path, "rb").read(); o = 0
    while o < len(b):
        n = int(np.frombuffer(b[o:o + 8], np.uint64)[0]); o += 8
        out.append(np.frombuffer(b[o:o + 32 * (2 * n - 1)], np.uint8).reshape(2 * n - 1, 32).copy()); o += 32 * (2 * n - 1)
    return out


def record_open(n, env, td, perturb):
    tag = "%d_%d" % (n, perturb)
    files = {k: os.path.join(td, "%s_%s.bin" % (k, tag)) for k in ("stream", "trees", "r12")}
    sec = os.path.join(td, "commit_%s.npy" % tag)
    t0 = time.time()
    p = run_child(["--child-open", n, sec], dict(env, HOBBIT_REC_STREAM=files["stream"], HOBBIT_PARITY_TREES=files["trees"], HOBBIT_PARITY_R12=files["r12"]), perturb, may_die=True)
    dt = time.time() - t0
    assert p.returncode != 0 and "UNEXPECTED" not in p.stdout, (p.returncode, p.stdout[-400:])
    assert "SHA3" in p.stderr, "the child should end on the unlinked SHA3: " + p.stderr[-400:]
    rec = np.fromfile(files["stream"], np.uint64).reshape(-1, 6)
    trees = read_trees(files["trees"])
    l = (2 * n).bit_length() - 1
    r12 = np.fromfile(files["r12"], np.uint64).reshape(2, l, 2)
    return dict(rec=rec, trees=trees, r1=r12[0], r2=r12[1], commit_seconds=float(np.load(sec)[0]), seconds=dt)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-lists":
        return child_lists(int(a[1]), a[2])
    if a and a[0] == "--child-dims":
        return child_dims(int(a[1]), a[2])
    if a and a[0] == "--child-open":
        return child_open(int(a[1]), a[2])
    if a and a[0] == "--child-batch":
        return child_batch(int(a[1]), int(a[2]), a[3])
    if not pyoracle.ref_available():
        sys.exit(__doc__)
    td = tempfile.mkdtemp()
    try:
        out = os.path.join(td, "ref")
        mk = ["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "OUT=" + out]
        # sumcheck.cpp without optimisation first; the second call finds that object up to date and builds the rest as oracle/_ref is built
        subprocess.check_call(mk + ["REFFLAGS=" + REFFLAGS.replace("-O3", "-O0"), os.path.join(out, "obj", "sumcheck.o")])
        subprocess.check_call(mk + [os.path.join(out, "libhobbit_ref.so")])
        rec_so = os.path.join(td, "libparity_recorder.so")
        subprocess.check_call(["g++", "-std=c++14"] + REFFLAGS.split() + ["-shared", "-o", rec_so, os.path.join(ROOT, "scripts", "parity_recorder.cpp")])
        env = dict(os.environ, HOBBIT_PM_MIMC_SO=os.path.join(ROOT, "oracle", "_ref", "libref_recorder_mimc.so"), HOBBIT_PM_RECORDER=rec_so,
                   HOBBIT_PM_REF_SO=os.path.join(out, "libhobbit_ref.so"))
        env.pop("MALLOC_PERTURB_", None)
        res = {"ns": np.array(NS), "batches": np.array(BATCHES), "malloc_perturb": np.array([255])}
        for n in NS:
            f_l, f_d = os.path.join(td, "lists_%d.npz" % n), os.path.join(td, "dims_%d.npz" % n)
            run_child(["--child-lists", n, f_l], env); run_child(["--child-dims", n, f_d], env)
            ls, dm = dict(np.load(f_l)), dict(np.load(f_d))
            assert np.array_equal(ls["dims"], dm["dims"]) and ls["total"][0] == dm["total"][0], "graph dimensions differ from oracle/_ref's at n = %d" % n
            o = record_open(n, env, td, 255)
            again = record_open(n, env, td, 255)
            assert np.array_equal(o["rec"], again["rec"]), "the MALLOC_PERTURB_=255 run does not reproduce itself"
            m = int(ls["m"][0]); P = 1 << (m - 1).bit_length()
            assert len(o["trees"]) >= 2 and o["trees"][0].shape[0] == 2 * P - 1 and o["trees"][1].shape[0] == 2 * (P // 4) - 1, [t.shape for t in o["trees"]]
            cp = o["trees"][0]; dgs, off, sz = [], 0, P
            while sz >= 1:
                dgs.append(dg(cp[off:off + sz])); off += sz; sz //= 2
            k = "_%d" % n
            res.update({"m" + k: ls["m"], "P" + k: np.array([P]), "dims" + k: ls["dims"], "idx1_dg" + k: ls["idx1_dg"], "idx2_dg" + k: ls["idx2_dg"], "weight_dg" + k: ls["weight_dg"],
                        "cp_root" + k: cp[-1].copy(), "cp_level_dg" + k: np.stack(dgs), "cw_root" + k: o["trees"][1][-1].copy(), "r1" + k: o["r1"], "r2" + k: o["r2"],
                        "transcript" + k: o["rec"], "ref_seconds" + k: np.array([o["commit_seconds"], o["seconds"]])})
            print("n = %d: m %d, P %d, %d records before SHA3, C_p root %s, reference commit %.2f s, child %.2f s" % (n, m, P, o["rec"].shape[0], cp[-1].tobytes().hex()[:16],
                                                                                                                   o["commit_seconds"], o["seconds"]), flush=True)
            if n == NS[0]:
                other = record_open(n, env, td, 85)
                k0 = min(o["rec"].shape[0], other["rec"].shape[0])
                diff = np.nonzero((o["rec"][:k0] != other["rec"][:k0]).any(axis=1))[0]
                assert len(diff), "the transcript does not depend on the allocator's fill byte any more"
                res["other_perturb"] = np.array([85]); res["other_first_diff"] = np.array([int(diff[0])]); res["other_cp_root_equal"] = np.array([int(np.array_equal(other["trees"][0], cp))])
                print("  MALLOC_PERTURB_=85: transcript differs from record %d on; C_p equal: %d" % (diff[0], res["other_cp_root_equal"][0]), flush=True)
        for n, count in BATCHES:
            f_b = os.path.join(td, "batch_%d_%d.npz" % (n, count))
            run_child(["--child-batch", n, count, f_b], env, 255)
            b = dict(np.load(f_b))
            for key, v in b.items():
                res["batch_%d_%d_%s" % (n, count, key)] = v
            print("batch (%d, %d): %d rounds, %.2f s" % (n, count, b["poly"].shape[0], float(b["ref_seconds"][0])), flush=True)
        name = os.path.join(GOLD, "parity_matrix.npz")
        np.savez_compressed(name, **res)
        print("%s: %d bytes" % (name, os.path.getsize(name)))
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
