"""scripts/gen_brakedown_stream_golden.py -- TEST INFRASTRUCTURE ONLY (runs where oracle/_ref can be built).

Fixtures of the streaming Brakedown baseline, test_Elastic_PC(N, 3) (src/Elastic_PC.cpp:784-806: commit_brakedown_stream :112-172,
open_brakedown_stream :561-623), recorded from the REAL reference.  As scripts/gen_brakedown_golden.py does (its docstring says why the
reference is rebuilt with -ffp-contract=off): scripts/brakedown_recorder.cpp -- the same recorder, the two drivers go through the same
Merkle entry points -- is compiled into a temporary directory and loaded in front of the reference in a fresh child process per shape
(call-through interposers on create_tree_blake / open_tree_blake / MT_commit_Blake, which sees every padded reply vector, and a stand-in for
verify_claim_opt_blake, which ends in SHA3).  The recorder is shared: a change made to it for test_PC option 3 changes what these fixtures
record too, so regenerate both sets after one.  A second fresh child replays the libc draws (expander_init_store(B), generate_randomness(n),
generate_randomness(1), 2935 x rand() % 2B) through the reference's own functions: its I must equal the recorded one, the replies must be
its encode of the stream's chunk at I, and the aggregates, which the inlined encode_monolithic leaves unobservable, are computed from those
inputs with the oracle's field ops.

Leaf 2B-1 of the reference's level 0 reads one element past two heap arrays (commit_input[0..1][2B]) and is undefined; it is an odd leaf of a
left|left tree and feeds no parent.  It is left out: the level-0 digest is over leaves [0, 2B-1).

  tests/golden/brakedown_stream_2e<n>.npz   B, chunks, root, sha256 of every level, sampled level-0 leaves, x, r0, I, replies (digest and
                                            samples), the opening path, both aggregates (digests and samples), ps

usage: python scripts/gen_brakedown_stream_golden.py 16 17 20 21 24
"""
import ctypes
import hashlib
import os
import re
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
QUERIES = 2935
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
    B = 1 << ((logn - 1) // 2 + 6)
    return B, (1 << logn) // B


def sample_plan(logn):
    """deterministic sample positions"""
    B, chunks = shape(logn)
    g = np.random.default_rng(7100 + logn)
    W = 2 * B
    leaves = g.integers(0, W - 1, NS); leaves[:3] = [0, 1, W - 2]
    rq = g.integers(0, QUERIES, NS); ri = g.integers(0, chunks, NS)
    aj = g.integers(0, B, NS); aj[:2] = [0, B - 1]
    return dict(leaves=leaves, rq=rq, ri=ri, aj=aj)


def level_dgs(lv, W):
    """sha256 of every level; level 0 over leaves [0, W-1) only"""
    out, off, sz = [], 0, W
    while sz >= 1:
        out.append(dg(lv[off:off + (sz - 1 if off == 0 else sz)])); off += sz; sz //= 2
    return np.stack(out)


def _libc():
    libc = ctypes.CDLL(None)
    libc.dlopen.restype = ctypes.c_void_p; libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libc.dlsym.restype = ctypes.c_void_p; libc.dlsym.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    libc.dlerror.restype = ctypes.c_char_p
    return libc


def child_record(logn, out_path):
    """fresh process: test_Elastic_PC(2^logn, 3) of the real reference with the recorder in front"""
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
    B, chunks = shape(logn); W = 2 * B
    t0 = time.time()
    ctypes.CFUNCTYPE(None, ctypes.c_size_t, ctypes.c_int)(libc.dlsym(h_ref, b"_Z15test_Elastic_PCmi"))(1 << logn, 3)
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
    assert rec.rec_reply_count() == nq and rec.rec_reply_len() == chunks
    reply = np.zeros((nq, chunks, 2), np.uint64); rec.rec_replies(reply.ctypes.data_as(ctypes.c_void_p))
    np.savez(out_path, levels=lv, I=I, paths=paths, reply=reply, ps_paths=np.array([rec.rec_ps_paths()]), ref_seconds=np.array([dt]))
    os._exit(0)


def child_replay(logn, out_path):
    """fresh process: the same libc draws through the reference's own functions, then the aggregates with the oracle's field ops"""
    pyoracle.REF_SO = os.environ["HOBBIT_BD_REF_SO"]
    ref = pyoracle.Ref()
    orc = pyoracle.Oracle()
    N = 1 << logn
    B, chunks = shape(logn); W = 2 * B
    ref.rng_reset()
    ref.expander_init_store(B)                         # the driver (:794)
    x = ref.generate_randomness(logn)                  # open_brakedown_stream's argument (:802)
    r0 = ref.generate_randomness(1)[0]                 # (:570)
    libc = ctypes.CDLL(None)
    I = np.array([libc.rand() % W for _ in range(QUERIES)], np.uint64)                       # (:576-578)
    chunk = ref.read_stream_pc(N, B, 0)
    for i in (1, chunks - 1):
        assert np.array_equal(ref.read_stream_pc(N, B, i), chunk), "every chunk of the default stream is the same vector"
    code, ln = ref.encode_monolithic(chunk)
    code[ln:] = 0
    beta = orc.precompute_beta(x[:chunks.bit_length() - 1])
    rv = np.zeros((chunks, 2), np.uint64); rv[0] = r0
    for i in range(1, chunks):
        rv[i] = orc.f_mul(rv[i - 1:i], rv[0:1])[0]
    ab = np.zeros((B, 2), np.uint64); ar = np.zeros((B, 2), np.uint64)
    for i in range(chunks):
        ab = orc.f_add(ab, orc.f_mul(np.broadcast_to(beta[i], (B, 2)), chunk))
        ar = orc.f_add(ar, orc.f_mul(np.broadcast_to(rv[i], (B, 2)), chunk))
    np.savez(out_path, x=x, r0=r0, I=I, aggr_beta=ab, aggr_r=ar, code_at_I=code[I.astype(np.int64)])
    os._exit(0)


def gen(logn, rec_so, ref_so, td):
    B, chunks = shape(logn); W = 2 * B
    env = dict(os.environ, HOBBIT_BD_RECORDER=rec_so, HOBBIT_BD_REF_SO=ref_so)
    f_rec = os.path.join(td, "rec_%d.npz" % logn)
    p = subprocess.run([sys.executable, __file__, "--child-record", str(logn), f_rec], capture_output=True, text=True, env=env, timeout=4 * 3600)
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-800:])
    stdout = p.stdout
    rec = dict(np.load(f_rec))
    lv = rec["levels"]
    sp = sample_plan(logn)
    out = {"B": np.array([B]), "chunks": np.array([chunks]), "root": lv[-1].copy(), "ref_seconds": rec["ref_seconds"]}
    out["level_dg"] = level_dgs(lv, W)
    out["leaves_idx"] = sp["leaves"]; out["leaves_s"] = lv[sp["leaves"]].copy()
    I = rec["I"]
    assert (rec["paths"] == rec["paths"][0]).all(), "every opening path should be leaf 0's"
    out["I"] = I.astype(np.uint32); out["path"] = rec["paths"][0].copy()
    out["reply_dg"] = dg(rec["reply"]); out["rq"] = sp["rq"]; out["ri"] = sp["ri"]; out["reply_s"] = rec["reply"][sp["rq"], sp["ri"]].copy()
    f_rp = os.path.join(td, "rp_%d.npz" % logn)
    q = subprocess.run([sys.executable, __file__, "--child-replay", str(logn), f_rp], capture_output=True, text=True, env=env, timeout=4 * 3600)
    assert q.returncode == 0, (q.returncode, q.stderr[-800:])
    rp = dict(np.load(f_rp))
    assert np.array_equal(rp["I"], I), "the replayed draws do not give the recorded queries"
    assert np.array_equal(rec["reply"], np.broadcast_to(rp["code_at_I"][:, None], rec["reply"].shape)), "replies are codeword_i[I[q]]"
    out["x"] = rp["x"]; out["r0"] = rp["r0"]
    out["aggr_beta_dg"] = dg(rp["aggr_beta"]); out["aggr_r_dg"] = dg(rp["aggr_r"])
    out["aj"] = sp["aj"]; out["aggr_beta_s"] = rp["aggr_beta"][sp["aj"]].copy(); out["aggr_r_s"] = rp["aggr_r"][sp["aj"]].copy()
    ps = float(rec["ps_paths"][0]) + QUERIES * chunks * 16 / 1024.0 + 2 * B * 16 / 1024.0
    m = re.search(r"^Ps : (\S+), Vt", stdout, re.M)
    assert m and m.group(1) == "%f" % ps, (stdout[-300:], ps)
    out["ps"] = np.array([ps]); out["ps_paths"] = rec["ps_paths"]
    name = os.path.join(GOLD, "brakedown_stream_2e%d.npz" % logn)
    np.savez_compressed(name, **out)
    print("2^%d: B %d, chunks %d, reference test_Elastic_PC(., 3) %.1f s, root %s, ps %f, %d bytes" % (
        logn, B, chunks, float(rec["ref_seconds"][0]), lv[-1].tobytes().hex(), ps, os.path.getsize(name)), flush=True)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-record":
        return child_record(int(a[1]), a[2])
    if a and a[0] == "--child-replay":
        return child_replay(int(a[1]), a[2])
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
            gen(n, rec_so, os.path.join(out, "libhobbit_ref.so"), td)
    finally:
        shutil.rmtree(td)


if __name__ == "__main__":
    main()
