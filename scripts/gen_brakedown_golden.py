"""scripts/gen_brakedown_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref exists).

Fixtures of the Brakedown comparison baseline, test_PC(N, 3, K) (src/Our_PC.cpp:794-805), recorded from the REAL reference built into
oracle/_ref.  scripts/brakedown_recorder.cpp is compiled into a temporary directory and loaded in front of the reference in a fresh child
process (call-through interposers on create_tree_blake / open_tree_blake / MT_commit_Blake, a stand-in for verify_claim_opt_blake, which
ends in SHA3).  The reference is compiled for this into the same temporary directory by oracle/Makefile's own recipe, with
-ffp-contract=off added: the reference's CMakeLists.txt passes no -O flag, so its n * (r - 1) - L (src/expanders.h:87) is a multiply and a
subtract, while oracle/_ref's -O3 -march=x86-64-v3 build contracts it into one FMA, which truncates D[3].R at n = 2^20 to 3517 instead of
3518 (9850 * 0.72 - 3574) and changes every encoded column past 1 329 932 of the 2^28 matrix.  A second fresh child replays the libc draws (generate_randomness(N), expander_init_store(B), generate_randomness(log2 N),
rows x random(), 2900 x rand() % 2B) through the reference's own functions: its I must equal the recorded one, and the aggregates, which
encode_monolithic's inlining leaves unobservable, are computed from those inputs with the oracle's field ops.

  tests/golden/brakedown_2e<n>.npz   n = 20, 21, 22, 24: levels (digest of each, root, sampled level-0 digests), whole-matrix digest and
                                     sampled entries, I, replies (digest and samples), the opening path, r, aggregates (digests and samples), ps
                                     n = 28 (`--commit-only`): the commitment only (root, digests of every level, sampled columns)

usage: python scripts/gen_brakedown_golden.py 20 21 22 24  |  python scripts/gen_brakedown_golden.py --commit-only 28
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
REC_SRC = os.path.join(ROOT, "scripts", "brakedown_recorder.cpp")
NS = 64
QUERIES = 2900
RTLD_LAZY, RTLD_GLOBAL = 0x1, 0x100
SYM = dict(
    mt=b"_ZN11merkle_tree18merkle_tree_prover15MT_commit_BlakeEPN5virgo12fieldElementERSt6vectorIS4_I5_hashSaIS5_EESaIS7_EEi",
    ct=b"_ZN11merkle_tree18merkle_tree_prover17create_tree_blakeEiRSt6vectorIS1_I5_hashSaIS2_EESaIS4_EEib",
    ot=b"_ZN11merkle_tree18merkle_tree_prover15open_tree_blakeERSt6vectorIS1_I5_hashSaIS2_EESaIS4_EES1_ImSaImEEi",
    vf=b"_ZN11merkle_tree20merkle_tree_verifier22verify_claim_opt_blakeERSt6vectorIS1_I5_hashSaIS2_EESaIS4_EEPKS2_iiPbRd",
)


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def shape(logn):
    B = 1 << (logn // 2 + 6) if logn % 2 == 0 else 1 << ((logn - 1) // 2 + 6)
    return B, (1 << logn) // B


def sample_plan(logn):
    """deterministic sample positions shared with the tests"""
    B, rows = shape(logn)
    g = np.random.default_rng(7000 + logn)
    W = 2 * B
    ent_i = g.integers(0, rows, NS); ent_c = g.integers(0, W, NS)
    ent_i[:4] = [0, rows - 1, 3, 4 % rows]; ent_c[:4] = [0, W - 1, B, B - 1]
    leaves = g.integers(0, W, NS); leaves[:3] = [0, 1, W - 1]
    cols = np.concatenate([[0, 1, B - 1, B], g.integers(0, W, 4)])
    rq = g.integers(0, QUERIES, NS); ri = g.integers(0, rows, NS)
    aj = g.integers(0, B, NS); aj[:2] = [0, B - 1]
    return dict(ent_i=ent_i, ent_c=ent_c, leaves=leaves, cols=cols, rq=rq, ri=ri, aj=aj)


def _libc():
    libc = ctypes.CDLL(None)
    libc.dlopen.restype = ctypes.c_void_p; libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libc.dlsym.restype = ctypes.c_void_p; libc.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    libc.dlerror.restype = ctypes.c_char_p
    return libc


def _tensor_rows(addr, rows, W):
    """the reference's global `tensor` (vector<vector<vector<F>>>): rows of tensor[0], each W F"""
    rd = lambda a: ctypes.c_uint64.from_address(a).value  # noqa: E731  (std::vector = begin, end, capacity)
    t0 = rd(addr)                      # &tensor[0]
    rbeg = rd(t0)                      # &tensor[0][0]
    assert (rd(t0 + 8) - rbeg) // 24 == rows
    out = np.zeros((rows, W, 2), np.uint64)
    for i in range(rows):
        b = rd(rbeg + 24 * i)
        assert (rd(rbeg + 24 * i + 8) - b) // 16 == W
        ctypes.memmove(out[i].ctypes.data, b, 16 * W)
    return out


def child_record(logn, out_path, commit_only):
    """fresh process: test_PC(2^logn, 3, 128) of the real reference with the recorder in front"""
    libc = _libc()
    rec_so = os.environ["HOBBIT_BD_RECORDER"]
    h_rec = libc.dlopen(rec_so.encode(), RTLD_LAZY | RTLD_GLOBAL)
    assert h_rec, libc.dlerror()
    h_ref = libc.dlopen(os.environ["HOBBIT_BD_REF_SO"].encode(), RTLD_LAZY | RTLD_GLOBAL)
    assert h_ref, libc.dlerror()
    for s in SYM.values():
        assert libc.dlsym(None, s) == libc.dlsym(h_rec, s) and libc.dlsym(h_rec, s), "symbol %s does not resolve to the recorder" % s.decode()
    nxt = [libc.dlsym(h_ref, SYM[k]) for k in ("mt", "ct", "ot")]
    assert all(nxt) and nxt[0] != libc.dlsym(h_rec, SYM["mt"])
    rec = ctypes.CDLL(rec_so)
    rec.rec_set_next.argtypes = [ctypes.c_void_p] * 3
    rec.rec_set_next(*nxt)
    ref = ctypes.CDLL(os.environ["HOBBIT_BD_REF_SO"])
    ref.ref_init(); ref.ref_rng_reset()
    N = 1 << logn
    B, rows = shape(logn); W = 2 * B
    t0 = time.time()
    ctypes.CFUNCTYPE(None, ctypes.c_size_t, ctypes.c_int, ctypes.c_int)(libc.dlsym(h_ref, b"_Z7test_PCmii"))(N, 3, 128)
    libc.fflush(None)
    dt = time.time() - t0
    for f in ("rec_leaves", "rec_queries", "rec_depth", "rec_reply_count", "rec_reply_len"):
        getattr(rec, f).restype = ctypes.c_size_t
    rec.rec_ps_paths.restype = ctypes.c_double
    assert rec.rec_leaves() == W
    lv = np.zeros((2 * W - 1, 32), np.uint8); rec.rec_levels(lv.ctypes.data_as(ctypes.c_void_p))
    nq, depth = rec.rec_queries(), rec.rec_depth()
    assert nq == QUERIES and depth == W.bit_length() - 1
    I = np.zeros(nq, np.uint64); rec.rec_I(I.ctypes.data_as(ctypes.c_void_p))
    paths = np.zeros((nq, depth, 32), np.uint8); rec.rec_paths(paths.ctypes.data_as(ctypes.c_void_p))
    assert rec.rec_reply_count() == nq and rec.rec_reply_len() == rows
    reply = np.zeros((nq, rows, 2), np.uint64); rec.rec_replies(reply.ctypes.data_as(ctypes.c_void_p))
    res = dict(levels=lv, I=I, paths=paths, reply=reply, ps_paths=np.array([rec.rec_ps_paths()]), ref_seconds=np.array([dt]))
    sp = sample_plan(logn)
    addr = libc.dlsym(h_ref, b"tensor")
    if commit_only:
        T = None
        rd = lambda a: ctypes.c_uint64.from_address(a).value  # noqa: E731
        rbeg = rd(rd(addr))
        cols = np.zeros((len(sp["cols"]), rows, 2), np.uint64)
        for i in range(rows):
            b = rd(rbeg + 24 * i)
            for k, c in enumerate(sp["cols"]):
                ctypes.memmove(cols[k, i].ctypes.data, b + 16 * int(c), 16)
        res["cols"] = cols
    else:
        T = _tensor_rows(addr, rows, W)
        res["T"] = T
    np.savez(out_path, **res)
    os._exit(0)


def child_replay(logn, out_path):
    """fresh process: the same libc draws through the reference's own functions, then the aggregates with the oracle's field ops"""
    pyoracle.REF_SO = os.environ["HOBBIT_BD_REF_SO"]
    ref = pyoracle.Ref()
    orc = pyoracle.Oracle()
    N = 1 << logn
    B, rows = shape(logn); W = 2 * B
    ref.rng_reset()
    poly = ref.generate_randomness(N)                  # test_PC (:758)
    ref.expander_init_store(B)                         # commit_standard_brakedown (:199-206)
    x = ref.generate_randomness(logn)                  # open_brakedown_standard's argument
    libc = ctypes.CDLL(None); libc.random.restype = ctypes.c_long
    r = np.zeros((rows, 2), np.uint64); r[:, 0] = [libc.random() for _ in range(rows)]          # (:449-451)
    I = np.array([libc.rand() % W for _ in range(QUERIES)], np.uint64)                       # (:458-461)
    lr = rows.bit_length() - 1
    beta = orc.precompute_beta(x[:lr])
    ab = np.zeros((B, 2), np.uint64); ar = np.zeros((B, 2), np.uint64)
    for i in range(rows):
        row = poly[i * B:(i + 1) * B]                  # the systematic part of tensor[0][i]
        ab = orc.f_add(ab, orc.f_mul(np.broadcast_to(beta[i], (B, 2)), row))
        ar = orc.f_add(ar, orc.f_mul(np.broadcast_to(r[i], (B, 2)), row))
    np.savez(out_path, x=x, r=r, I=I, aggr_beta=ab, aggr_r=ar, poly_dg=dg(poly))
    os._exit(0)


def gen(logn, commit_only, rec_so, ref_so, td):
    B, rows = shape(logn); W = 2 * B
    env = dict(os.environ, HOBBIT_BD_RECORDER=rec_so, HOBBIT_BD_REF_SO=ref_so)
    f_rec = os.path.join(td, "rec_%d.npz" % logn)
    p = subprocess.run([sys.executable, __file__, "--child-record", str(logn), f_rec] + (["--commit-only"] if commit_only else []),
                       capture_output=True, text=True, env=env, timeout=4 * 3600)
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-800:])
    stdout = p.stdout
    rec = dict(np.load(f_rec))
    lv = rec["levels"]
    sp = sample_plan(logn)
    out = {"B": np.array([B]), "rows": np.array([rows]), "root": lv[-1].copy(), "ref_seconds": rec["ref_seconds"]}
    dgs, off, sz = [], 0, W
    while sz >= 1:
        dgs.append(dg(lv[off:off + sz])); off += sz; sz //= 2
    out["level_dg"] = np.stack(dgs)
    out["leaves_idx"] = sp["leaves"]; out["leaves_s"] = lv[sp["leaves"]].copy()
    out["stdout_commit"] = np.array([l for l in stdout.splitlines() if l.startswith("Commit time")][:1] or [""])
    if commit_only:
        out["cols_idx"] = sp["cols"]; out["cols"] = rec["cols"]
    else:
        T = rec["T"]
        out["T_dg"] = dg(T)
        out["ent_i"] = sp["ent_i"]; out["ent_c"] = sp["ent_c"]; out["ent"] = T[sp["ent_i"], sp["ent_c"]].copy()
        I = rec["I"]
        assert (rec["paths"] == rec["paths"][0]).all(), "every opening path should be leaf 0's"
        out["I"] = I.astype(np.uint32); out["path"] = rec["paths"][0].copy()
        out["reply_dg"] = dg(rec["reply"]); out["rq"] = sp["rq"]; out["ri"] = sp["ri"]; out["reply_s"] = rec["reply"][sp["rq"], sp["ri"]].copy()
        assert np.array_equal(rec["reply"], T[:, I.astype(np.int64)].transpose(1, 0, 2)), "replies are T[i][I[q]]"
        # replay: the draws and the aggregates
        f_rp = os.path.join(td, "rp_%d.npz" % logn)
        q = subprocess.run([sys.executable, __file__, "--child-replay", str(logn), f_rp], capture_output=True, text=True, env=env, timeout=4 * 3600)
        assert q.returncode == 0, (q.returncode, q.stderr[-800:])
        rp = dict(np.load(f_rp))
        assert np.array_equal(rp["I"], I), "the replayed draws do not give the recorded queries"
        assert np.array_equal(dg(T[:, :B].reshape(-1, 2)), rp["poly_dg"]), "tensor[0][i][0..B) is row i of the replayed polynomial"
        out["x"] = rp["x"]; out["r"] = rp["r"]
        out["aggr_beta_dg"] = dg(rp["aggr_beta"]); out["aggr_r_dg"] = dg(rp["aggr_r"])
        out["aj"] = sp["aj"]; out["aggr_beta_s"] = rp["aggr_beta"][sp["aj"]].copy(); out["aggr_r_s"] = rp["aggr_r"][sp["aj"]].copy()
        ps = float(rec["ps_paths"][0]) + QUERIES * rows * 16 / 1024.0 + float((2 * B * 16) // 1024)
        out["ps"] = np.array([ps]); out["ps_paths"] = rec["ps_paths"]
        out["stdout_open"] = np.array([l.split("ps = ")[0] for l in stdout.splitlines() if l.startswith("PC Open")][:1] or [""])
    name = os.path.join(GOLD, "brakedown_2e%d.npz" % logn)
    np.savez_compressed(name, **out)
    print("2^%d: B %d, rows %d, reference test_PC %.1f s, root %s, %d bytes" % (logn, B, rows, float(rec["ref_seconds"][0]), lv[-1].tobytes().hex(),
                                                                                   os.path.getsize(name)), flush=True)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-record":
        return child_record(int(a[1]), a[2], "--commit-only" in a)
    if a and a[0] == "--child-replay":
        return child_replay(int(a[1]), a[2])
    commit_only = "--commit-only" in a
    ns = [int(v) for v in a if not v.startswith("--")]
    if not ns or not pyoracle.ref_available():
        sys.exit(__doc__)
    td = tempfile.mkdtemp()
    try:
        rec_so = os.path.join(td, "libbrakedown_recorder.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", rec_so, REC_SRC])
        out = os.path.join(td, "ref")
        flags = "-O3 -DNDEBUG -w -fPIC -march=x86-64-v3 -msha -mavx -ffp-contract=off -I$(REF)/src -idirafter /opt/conda/include"
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "OUT=" + out, "REFFLAGS=" + flags, os.path.join(out, "libhobbit_ref.so")])
        for n in ns:
            gen(n, commit_only, rec_so, os.path.join(out, "libhobbit_ref.so"), td)
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
