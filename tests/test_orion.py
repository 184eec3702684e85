"""The Orion comparison baseline, test_PC(N, 2, K) (include/hobbit_orion.h; reference src/Our_PC.cpp:28-65 _compute_tensorcode_linear_code,
173-195 commit_standard_orion, 523-602 open_orion_standard, 780-793 the driver; src/PC_utils.cpp:150-166 recursive_prover_orion).

Three layers of evidence, as for Braking base (tests/test_brakingbase.py):
  * tests/golden/orion.npz -- the REAL reference's own test_PC(2^n, 2, 128) (scripts/gen_orion_golden.py), as far as it can run;
  * tests/orion_model.py -- the whole flow restated from the oracle's pieces, pinned on the CPU by tests/test_orion_model_cpu.py;
  * the device (here, -m gpu): every output against the model at n = 14, 16, 18, 20, the library's own transcript recorder against the
    fixture; at n = 24 -- the first shape whose Q is capped at 4096 < B -- device against device, with no oracle run of that size.
Every input lies on the libc stream of a fresh process running test_PC(N, 2, .): srandom(1), the polynomial, the graphs of n = B, x.
"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import orion_model as om
from test_parity_matrix import Transcript, peek_randomness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "orion.npz")
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
SHAPES = (14, 16, 18, 20)
libc = ctypes.CDLL(None)
libc.random.restype = ctypes.c_long
V, S = ctypes.c_void_p, ctypes.c_size_t


def dg(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def level_dgs(flat, n):
    out, off, sz = [], 0, n
    while sz >= 1:
        out.append(dg(flat[off:off + sz])); off += sz; sz //= 2
    return np.stack(out)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def _mod():
    from __graft_entry__ import load_package
    return load_package()


def model_open(orc, logn):
    return om.model_open(orc, logn, Transcript, peek_randomness)


# ---- the header and its symbols (CPU) -------------------------------------------------------------------------------------------------------------
ASYNC = {"hobbit_orion_commit", "hobbit_encode_interleaved_ld", "hobbit_encode_interleaved_ld_order"}
HOST_RETURNING = {"hobbit_orion_open", "hobbit_orion_root", "hobbit_orion_gather", "hobbit_orion_grid_paths"}
EXEMPT = {
    "hobbit_orion_shape": "host only",
    "hobbit_orion_free": "free function: waits for the stream",
    "hobbit_orion_dims": "accessor, host only",
    "hobbit_orion_tensor_dev": "accessor of a raw device pointer",
    "hobbit_orion_levels_dev": "accessor of a raw device pointer",
    "hobbit_orion_proof_size": "host only: accounting over host buffers",
}


def declared(header="hobbit_orion.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    from __graft_entry__ import build_hip
    build_hip()
    mod = _mod()
    lib = mod.load_library()
    decl = declared()
    assert len(decl) == 13 and sorted(mod.ORION_SYMBOLS) == decl
    for s in decl:
        assert hasattr(lib, s), "missing export " + s
        assert getattr(lib, s).argtypes is not None, "no prototype bound for " + s
    for other in (mod.ABI_SYMBOLS, mod.PARITY_SYMBOLS, mod.WHIR_SYMBOLS, mod.BRAKINGBASE_SYMBOLS):
        assert not set(decl) & set(other)
    for header in ("hobbit_hip.h", "hobbit_parity.h", "hobbit_whir.h", "hobbit_brakingbase.h"):
        assert not [s for s in declared(header) if "orion" in s or "interleaved_ld" in s], header
    for meth in ("orion_shape", "orion_commit", "orion_open", "orion_gather", "orion_grid_paths", "encode_interleaved_ld"):
        assert callable(getattr(mod.Hobbit, meth))
    for meth in ("root", "levels", "tensor", "open", "free"):
        assert callable(getattr(mod.OrionCommitment, meth))


def test_every_export_is_classified():
    """what tests/test_async_contract.py asks of hobbit_hip.h, for the fifth header: asynchronous (with a stream test below), host-returning or exempt"""
    sets = {"ASYNC": ASYNC, "HOST_RETURNING": HOST_RETURNING, "EXEMPT": set(EXEMPT)}
    names = set(declared())
    for n in sorted(names):
        assert len([k for k, s in sets.items() if n in s]) == 1, n
    for k, s in sets.items():
        assert not (s - names), (k, sorted(s - names))


def test_shape_limits():
    from __graft_entry__ import build_hip
    build_hip()
    hb = _mod()
    assert hb.Hobbit.orion_shape(1 << 14) == (128, 128) and hb.Hobbit.orion_shape(1 << 24) == (4096, 4096)
    assert hb.Hobbit.orion_shape(1 << 26) == (8192, 4096) and hb.Hobbit.orion_shape(1 << 28) == (16384, 4096)
    for N in (1 << 12, 1 << 15, 1 << 27, 1 << 29, 1 << 30, 3 << 14, (1 << 16) + 1, 0, 1):
        with pytest.raises(hb.HobbitError):
            hb.Hobbit.orion_shape(N)


def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


def test_host_test_pc_refusals():
    """shapes outside the range end with status 255 before anything is drawn or any device is opened; `test_pc <n> 2 <K>` keeps refusing"""
    from __graft_entry__ import build_hip, build_host
    build_hip(); build_host()
    for args in (("orion", 12), ("orion", 15), ("orion", 30), ("orion", 0)):
        p = _test_pc(args, 120)
        assert p.returncode == 255 and "Error: Orion" in p.stdout and "root" not in p.stdout, (args, p.returncode, p.stdout[-300:])
    p = _test_pc((20, 2, 128), 120)
    assert p.returncode == 255 and "comparison baseline" in p.stdout, (p.returncode, p.stdout[-300:])


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)
    yield h
    h.close()


def same(a, b, what):
    if isinstance(b, dict):
        for k in b:
            same(a[k], b[k], what + "/" + k)
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def same_opening(got, want):
    for k in ("I", "J", "c_root", "cp_root", "p1", "checks", "sp_c", "ps"):
        same(got[k], want[k], k)
    for k in ("t1", "t2", "p2", "p3", "p4", "cw_root", "scalars", "partial", "acc_y", "checks", "sp_p", "sp_w"):
        same(got["parity"][k], want["parity"][k], "parity/" + k)


def device_commit(hb, orc, logn):
    poly, x = om.begin(orc, logn)
    B = om.shape(1 << logn)[0]
    hb.upload_graphs(B, om.graphs(orc, B))
    return hb.orion_commit(poly), x


def check_commit(c, C, gold, logn):
    assert (c.N, c.B, c.Q, c.len) == (C["N"], C["B"], C["Q"], C["len"])
    lv = c.levels()
    assert np.array_equal(lv, C["levels"]) and np.array_equal(c.root(), C["root"])
    T = c.tensor()
    bad = np.argwhere((T != C["T"]).any(axis=2))
    assert not len(bad), ("tensor entries that differ from the model (row, column)", bad[:8].tolist(), len(bad))
    assert np.array_equal(c.tensor(C["B"] - 1, 3), C["T"][C["B"] - 1:C["B"] + 2])
    k = "_%d" % logn
    assert np.array_equal(c.root(), gold["root" + k]) and np.array_equal(level_dgs(lv, c.N), gold["level_dg" + k])
    assert np.array_equal(dg(T), gold["T_dg" + k])
    assert np.array_equal(T[:, gold["cols_idx" + k]].transpose(1, 0, 2), gold["cols" + k])


@pytest.mark.gpu
@pytest.mark.parametrize("logn", SHAPES)
def test_commit_on_the_device(hb, oracle, gold, logn):
    """every level, the root and the whole tensor against the model and the fixture"""
    c, _ = device_commit(hb, oracle, logn)
    check_commit(c, om.model_commit(oracle, logn), gold, logn)
    c.free()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", (14, 16))
def test_commit_writes_every_entry_of_a_dirty_buffer(hb, oracle, gold, logn):
    """the allocator hands a freed buffer of the same size out again: eight such buffers are filled with 0xFF and parked, the commitment takes
    its tensor from them, and every one of its 4N entries is the model's -- the zero blocks nobody encodes included"""
    poly, _ = om.begin(oracle, logn)
    B = om.shape(1 << logn)[0]
    hb.upload_graphs(B, om.graphs(oracle, B))
    nbytes = 4 * (1 << logn) * 16
    bufs = [hb.alloc(nbytes) for _ in range(8)]
    ptrs = {b.ptr for b in bufs}
    for b in bufs:
        hb._chk(hb.lib.hobbit_memset(hb.ctx, b.ptr, 0xFF, nbytes))
    hb.sync()
    for b in bufs:
        b.free()
    c = hb.orion_commit(poly)
    assert c.tensor_ptr in ptrs, "the commitment did not take a dirtied buffer: the test shows nothing"
    check_commit(c, om.model_commit(oracle, logn), gold, logn)
    c.free()


def read_paths(hb, buf, pairs, depth):
    return np.stack([hb.to_host(buf, (depth, 32), np.uint8, offset=int(p) * depth * 32) for p in pairs])


@pytest.mark.gpu
@pytest.mark.parametrize("logn", SHAPES)
def test_open_on_the_device(hb, oracle, gold, logn):
    """every output against the model, both checks hold, the library's own transcript equals the real reference's record for record over the
    fixture's length and goes on past it; the paths complete at n = 14 and 16, first, last and a few hundred sampled pairs at 18 and 20"""
    want = model_open(oracle, logn)
    C = om.model_commit(oracle, logn)
    c, x = device_commit(hb, oracle, logn)
    assert np.array_equal(x, want["x"])
    hb.lib.hobbit_transcript_record(1)
    try:
        got = c.open(x)
        cnt = hb.lib.hobbit_transcript_count()
        rec = np.zeros((cnt, 6), np.uint64)
        hb.lib.hobbit_transcript_read(rec.ctypes.data_as(ctypes.c_void_p), cnt)
    finally:
        hb.lib.hobbit_transcript_record(0)
    assert got["checks"].tolist() == [1, 1]
    same_opening(got, want["open"])
    k = "_%d" % logn
    ref = gold["transcript" + k]
    assert cnt > ref.shape[0]
    bad = np.nonzero((rec[:ref.shape[0]] != ref).any(axis=1))[0]
    assert not len(bad), "first differing record: %d" % bad[0]
    assert np.array_equal(got["I"], gold["I" + k]) and np.array_equal(got["J"], gold["J" + k])
    assert np.array_equal(got["c_root"], gold["c_root" + k]) and np.array_equal(got["cp_root"], gold["cp_root" + k])
    assert np.array_equal(got["parity"]["cw_root"], gold["cw_root" + k])
    Q, depth = c.Q, logn
    if logn <= 16:
        paths = hb.to_host(got["paths"], (Q * Q, depth, 32), np.uint8)
        assert np.array_equal(paths, om.paths(C, want["open"]))
    else:
        pairs = np.concatenate([[0, Q * Q - 1, Q - 1, Q * (Q - 1)], np.random.default_rng(logn).integers(0, Q * Q, 300)])
        assert np.array_equal(read_paths(hb, got["paths"], pairs, depth), om.paths(C, want["open"], pairs))
    c.free()


def next_draws(seed, k=4):
    libc.srandom(seed)
    return [libc.random() for _ in range(k)]


@pytest.mark.gpu
def test_refusals(hb, oracle):
    """n = 12, 15, 30, N not a power of two, graphs finalized for another n: each returns its code with the libc stream untouched and nothing
    launched"""
    mod = _mod()
    poly, x = om.begin(oracle, 14)
    hb.upload_graphs(128, om.graphs(oracle, 128))
    d = hb.to_device(poly)
    c = hb.orion_commit((d, 1 << 14))
    want = next_draws(5)
    libc.srandom(5)
    hb.profile(True); hb.profile_reset()
    try:
        for N in (1 << 12, 1 << 15, 1 << 30, 3 << 13, (1 << 14) + 4):
            h = V()
            rc = hb.lib.hobbit_orion_commit(hb.ctx, V(d.ptr), S(N), ctypes.byref(h))
            assert rc == -2 and not h.value, (N, rc)
        h = V()
        assert hb.lib.hobbit_orion_commit(hb.ctx, V(d.ptr), S(1 << 16), ctypes.byref(h)) == -5 and not h.value        # B = 256: graphs finalized for another n
        o = (V * 14)()
        assert hb.lib.hobbit_orion_open(hb.ctx, c.h, V(x.ctypes.data), 14, o) == -2                                    # parity and sp_c are required
        assert hb.lib.hobbit_orion_open(hb.ctx, None, V(x.ctypes.data), 14, o) == -2
        om.start(oracle, 1 << 16); hb.upload_graphs(256, om.graphs(oracle, 256))                                       # (the oracle draws; this process' libc is reset below)
        libc.srandom(5)
        with pytest.raises(mod.HobbitError, match="rc=-5"):
            c.open(x)                                                                                                  # the graphs have moved on since the commitment
        ran = set(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()
    assert [libc.random() for _ in range(4)] == want, "a refused call drew from libc"
    assert not {k for k in ran if "orion" in k or "enc" in k or "blake" in k or "merkle" in k}, ran
    c.free()


# ---- n = 24: Q = 4096 < B, device against device ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capped_queries_at_2e24(hb, oracle):
    """N = 2^24 (B = 4096 = Q: the first shape on the capped branch of the query count), a polynomial filled on the device, no oracle run of the
    size.  Sampled rows and columns of the tensor equal hobbit_encode_batch of the same inputs; the gathered queried columns equal a read-back
    of the tensor's rows, and their commitment is the opening's C; sampled paths equal hobbit_merkle_paths; both checks of the opening hold"""
    import adversarial as A
    logn, N, B, Q = 24, 1 << 24, 4096, 4096
    W = 2 * B
    hb.upload_graphs(B, A.drawn_graphs(oracle, B))
    d = hb.fill_splitmix(N, 2424)
    c = hb.orion_commit((d, N))
    assert (c.B, c.Q) == (B, Q) and B < c.len < W
    g = np.random.default_rng(24)
    # rows: T[i] = encode(poly row i)
    rows = np.concatenate([[0, B - 1], g.integers(0, B, 6)])
    for i in rows:
        msg = hb.to_host(d, (B, 2), np.uint64, offset=int(i) * B * 16)
        assert np.array_equal(c.tensor(int(i), 1)[0], hb.encode_monolithic(msg)), int(i)
    # the gather against a read-back of whole rows
    libc.srandom(2424)
    got = c.open(hb.generate_randomness(logn))
    assert got["checks"].tolist() == [1, 1]
    I, J = got["I"], got["J"]
    assert len(I) == Q and I.max() < W and J.max() < W and len(set(I.tolist())) < Q
    arr = hb.alloc(Q * W * 16)
    hb._chk(hb.lib.hobbit_orion_gather(hb.ctx, V(c.tensor_ptr), S(W), S(W), V(I.ctypes.data), S(Q), V(arr.ptr)))
    qs = np.concatenate([[0, Q - 1], g.integers(0, Q, 30)]); cs = np.concatenate([[0, B - 1, B, c.len - 1, c.len, W - 1], g.integers(0, W, 26)])
    arr_rows = np.stack([hb.to_host(arr, (W, 2), np.uint64, offset=int(q) * W * 16) for q in qs])              # arr[q][:]
    T_rows = np.stack([c.tensor(int(r), 1)[0] for r in cs])                                                       # T[c][:]
    assert np.array_equal(arr_rows[:, cs], T_rows[:, I[qs].astype(np.int64)].transpose(1, 0, 2))
    # columns: a queried column is the codeword of its own first B entries (what the reference re-encodes), zeros behind
    for k, q in enumerate(qs[:8]):
        assert np.array_equal(arr_rows[k], hb.encode_monolithic(arr_rows[k][:B])), int(q)
    assert not arr_rows[:, c.len:].any() and arr_rows[:, B:c.len].any()
    enc = hb.alloc(2 * Q * W * 16); lv = hb.alloc(64 * (Q * W // 16))
    hb._chk(hb.lib.hobbit_shockwave_commit(hb.ctx, V(arr.ptr), S(Q * W), 32, V(enc.ptr), V(lv.ptr)))
    assert np.array_equal(hb.to_host(lv, (32,), np.uint8, offset=32 * (2 * (Q * W // 16) - 2)), got["c_root"])
    # paths
    pairs = np.concatenate([[0, Q * Q - 1, Q - 1, Q * (Q - 1)], g.integers(0, Q * Q, 300)])
    pos = ((J[pairs % Q].astype(np.uint64) // 4) * W + I[pairs // Q].astype(np.uint64))
    want = np.zeros((len(pairs), logn, 32), np.uint8)
    hb._chk(hb.lib.hobbit_merkle_paths(hb.ctx, V(c.levels_ptr), S(N), V(pos.ctypes.data), S(len(pos)), V(want.ctypes.data)))
    assert np.array_equal(read_paths(hb, got["paths"], pairs, logn), want)
    assert got["ps"] > (1 << 20) * 16 / 1024.0
    c.free()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mirror_and_cli(oracle, gold):
    """host/test_pc orion 16 in a child process: the reference's root, its lines, and the model's ps"""
    from __graft_entry__ import build_host
    build_host()
    want = model_open(oracle, 16)["open"]
    p = _test_pc(("orion", 16), 300)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    assert re.search(r"^OK$", p.stdout, re.M) and re.search(r"^256,512$", p.stdout, re.M), p.stdout[-500:]
    m = re.search(r"^root ([0-9a-f]{64})$", p.stdout, re.M)
    assert m and m.group(1) == bytes(gold["root_16"]).hex(), p.stdout[-500:]
    assert re.search(r"^Commit time: \S+ seconds$", p.stdout, re.M) and re.search(r"^Total time: \S+ seconds$", p.stdout, re.M)
    m = re.search(r"^ ps = (\S+), vt = \S+$", p.stdout, re.M)
    assert m and m.group(1) == "%f" % want["ps"], (p.stdout[-500:], want["ps"])


# ---- the stream contract: hobbit_orion_commit is asynchronous -------------------------------------------------------------------------------------------
BACKLOG_REPS, BACKLOG_N = 1000, 1 << 24      # the backlog of tests/test_async_contract.py: about 160 ms of element-wise products on the device


@pytest.mark.gpu
def test_commit_queued_behind_a_backlog_then_opened(hb, oracle):
    """commit on a caller's (torch) stream behind a backlog, the opening right behind it with no synchronisation in between: the bits of the
    synchronised run on the library's own stream"""
    import torch
    logn = 14
    B = om.shape(1 << logn)[0]
    poly, x = om.begin(oracle, logn); levels = om.graphs(oracle, B)
    hb.upload_graphs(B, levels)
    c = hb.orion_commit(poly)
    libc.srandom(77); want = c.open(x, want_paths=False); root = c.root(); lv = c.levels(); c.free()
    stream = torch.cuda.Stream()
    hs = _mod().Hobbit(0, stream=stream.cuda_stream)
    try:
        hs.upload_graphs(B, levels)
        d = hs.to_device(poly)
        w = hs.orion_commit((d, 1 << logn)); libc.srandom(3); w.open(x, want_paths=False); w.free()             # the shapes once: workspaces grow now
        t = [torch.empty((BACKLOG_N, 2), dtype=torch.int64, device="cuda") for _ in range(3)]
        for i in range(2):
            hs._chk(hs.lib.hobbit_fill_splitmix(hs.ctx, t[i].data_ptr(), BACKLOG_N, 77 + i))
        hs.sync()
        for _ in range(BACKLOG_REPS):
            hs._chk(hs.lib.hobbit_f_binop(hs.ctx, 2, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), BACKLOG_N))
        c2 = hs.orion_commit((d, 1 << logn), sync=False)
        busy = not stream.query()
        libc.srandom(77); got = c2.open(x, want_paths=False)
        assert np.array_equal(c2.root(), root) and np.array_equal(c2.levels(), lv)
        for k in ("I", "J", "c_root", "cp_root", "p1", "checks", "sp_c", "ps"):
            same(got[k], want[k], k)
        assert busy, "the commit returned to an idle stream: it waited, or the backlog is too short"
        c2.free()
    finally:
        hs.close()
