"""Timings of the other BASELINE.json configs on one MI355X (the north-star line is bench.py):
  C2  2-product sumcheck over 2^24 elements           (scripts/bench_sumcheck.py has the per-kernel view)
  C3  Our_PC commit of 2^26 coefficients (K = 32)
  C4  the MLP prover's math phases at MLP_test.sh's shape (B = 2^18, circuit 2^20: src/main.cpp:862-887) on synthetic resident streams:
      Elastic commit of the 4 * 2^20 witness (RS x RS), prove_multiplication_tree_stream_shallow(8 vectors x 2^20, distance 5),
      prove_gate_consistency over 2^20 gates, Elastic open.  The witness generator (Seval + witness_stream.cpp) is out of scope: what is
      timed is everything the prover computes once a chunk is in HBM (the reference spends 2.4-2.8 s of its 14 s there).
  C5  Elastic_PC streaming commit of 2^30 coefficients, B = 2^20, opt 1 and 2, on ONE GPU (chunks generated on the device side once:
      the reference's default stream repeats the same chunk, src/witness_stream.cpp:2405-2411), and the option-1 open (N = 2^26 too)
Prints one JSON object."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from __graft_entry__ import load_package

mod = load_package(); hb = mod.Hobbit(0)
splitmix_field = mod.splitmix_field
out = {}

def timed(fn, reps=3, warm=1):
    for _ in range(warm): fn()
    hb.sync(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    hb.sync(); return (time.perf_counter() - t0) / reps

# PM  the code's parity matrix (include/hobbit_parity.h): commit_parity_matrix and open_parity_matrix at n = 4096, 2^17 and 2^20.  Per stage
#     (host wall times of hobbit_parity_open, every stage ends synchronised), the host seconds of the list building, the launch count of
#     one opening and the gather kernel's achieved bytes per second (16 B of lists read and 96 B written per entry, the 32 B of gathered
#     table entries not counted) from the library's event brackets, next to the 8 TB/s this repository uses as peak.  The reference's CPU
#     seconds are those of tests/golden/parity_matrix.npz (n = 4096 only: commit, and the opening up to its first SHA3 call).
#     `python scripts/bench_configs.py parity [n ...]` runs this entry alone; `parity-gather n` one commit and one opening without
#     the event brackets, for a kernel trace of its own.  "commit_builders": the commit with the lists built on the host and by kernels
#     (include/hobbit_parity_lists.h), same graphs, same process.
def parity_builders(n, reps=3):
    """the parity commitment of the finalized code of n with the lists built on the host (hobbit_parity_commit) and by kernels
    (hobbit_parity_commit_device): wall time from the call to a synchronised stream, median of `reps` after one warm-up; the device builder's
    first call after the finalize (it uploads the code's forward form) on its own"""
    def wall(fn):
        hb.sync(); t0 = time.perf_counter(); pc = fn(n); hb.sync(); t = 1e3 * (time.perf_counter() - t0)
        root, sec = bytes(pc.root()).hex(), pc.list_seconds; pc.free()
        return t, root, sec
    wall(hb.commit_parity_matrix)
    host = [wall(hb.commit_parity_matrix) for _ in range(reps)]
    first = wall(hb.commit_parity_matrix_device)
    dev = [wall(hb.commit_parity_matrix_device) for _ in range(reps)]
    assert len(set(r[1] for r in host + [first] + dev)) == 1, "the two builders' roots differ"
    return dict(host_built=dict(ms=float(np.median([r[0] for r in host])), runs=[r[0] for r in host], lists_host_s=host[-1][2]),
                device_built=dict(first_call_ms=first[0], first_call_until_queued_s=first[2], ms=float(np.median([r[0] for r in dev])), runs=[r[0] for r in dev],
                                  until_queued_s=dev[-1][2]))

def parity_entry(ns=(4096, 1 << 17, 1 << 20), bare=False):
    res = {}
    gold = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "parity_matrix.npz"))
    for n in ns:
        hb.rng_reset(); t0 = time.perf_counter(); hb.expander_init_store(n); t_graphs = time.perf_counter() - t0
        l = (2 * n).bit_length() - 1
        r1, r2 = hb.generate_randomness(l), hb.generate_randomness(l)
        pc = hb.commit_parity_matrix(n); hb.sync(); pc.free()                                  # warm: workspaces, tables
        t0 = time.perf_counter(); pc = hb.commit_parity_matrix(n); hb.sync(); t_commit = time.perf_counter() - t0
        g = hb.open_parity_matrix(pc, r1, r2)                                                  # warm
        if not bare:
            hb.profile(True); hb.profile_reset()
        t0 = time.perf_counter(); g = hb.open_parity_matrix(pc, r1, r2); t_open = time.perf_counter() - t0
        assert g["checks"].tolist() == [1, 1]
        if bare:                                                                               # the list kernels, for the same trace: first call and a later one
            for _ in range(2):
                pd = hb.commit_parity_matrix_device(n); hb.sync(); pd.free()
        e = dict(m=pc.m, P=pc.P, graphs_host_draw_s=t_graphs, lists_host_s=pc.list_seconds, commit_ms=1e3 * t_commit, open_ms=1e3 * t_open,
                 stage_ms=dict(zip(("gather_and_Cw", "tree1", "eval_and_tree2", "sumchecks_P2_P3_P4", "shockwave_prove_Cp", "shockwave_prove_Cw"), g["stage_ms"].tolist())))
        if not bare:
            rep = hb.profile_report(); hb.profile(False)
            e["launches"] = int(sum(v[1] for v in rep.values()))
            ms = rep.get("k_parity_gather", (0.0, 0))[0]
            e["gather_ms"] = ms
            if ms:
                e["gather_bytes_per_s"] = 112.0 * pc.P / (1e-3 * ms); e["gather_fraction_of_8TBs"] = e["gather_bytes_per_s"] / 8e12
            e["commit_builders"] = parity_builders(n)
        if "ref_seconds_%d" % n in gold:
            e["reference_cpu_s"] = dict(commit=float(gold["ref_seconds_%d" % n][0]), open_child_until_first_sha3=float(gold["ref_seconds_%d" % n][1]))
        res["PM_n%d" % n] = e
        pc.free()
    return res

# WH  the standalone WHIR baseline (include/hobbit_whir.h; test_PC's last branch): hobbit_whir_commit and hobbit_whir_prove_any at 2^20, 2^22,
#     2^24, 2^26 between device events, warmed, the profiler off; at sizes hobbit_whir_prove serves, the two proofs alternated in one process
#     (materialised eq tables against the table-free out-of-domain step); then one run with the library's event brackets for the two new
#     kernels, against their products (R cur each per iteration) and their bytes (poly once; beta read and written once; the high tables).
#     `python scripts/bench_configs.py whir [logN ...]` runs this entry alone; `whir-bare logN` one warmed commit + proof and nothing else,
#     for a kernel trace of its own.
def whir_entry(logs=(20, 22, 24, 26), reps=5, bare=False):
    res = {}
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), runs=[float(t) for t in v])
    for logN in logs:
        N = 1 << logN
        d = hb.fill_splitmix(N, 5); x = splitmix_field(logN, 6); com, lv = hb.alloc(32 * N), hb.alloc(32 * N)
        commit = lambda: hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N, com.ptr, lv.ptr))
        def ev(fn):
            hb.timer_begin(); fn(); return hb.timer_end_ms()
        commit(); r = hb.whir_prove_any((d, N), x, com, lv); assert r["checks"].tolist() == [1, 1]           # warm: workspaces, twiddles
        if bare:
            hb.sync(); commit(); hb.whir_prove_any((d, N), x, com, lv); continue
        e = dict(commit_ms=stat([ev(commit) for _ in range(reps)]), iters=int(r["iters"][0]))
        if logN <= 24:
            hb.whir_prove((d, N), x, com, lv)                                                               # warm the other form's scratch
            ta, tb = [], []
            for _ in range(reps):
                ta.append(ev(lambda: hb.whir_prove((d, N), x, com, lv))); tb.append(ev(lambda: hb.whir_prove_any((d, N), x, com, lv)))
            e["prove_tables_ms"] = stat(ta); e["prove_any_ms"] = stat(tb)
        else:
            e["prove_any_ms"] = stat([ev(lambda: hb.whir_prove_any((d, N), x, com, lv)) for _ in range(reps)])
        hb.profile(True); hb.profile_reset(); hb.whir_prove_any((d, N), x, com, lv); rep = hb.profile_report(); hb.profile(False); hb.profile_reset()
        prod = by_y = by_b = 0; R, t = 100, 1
        while logN - 4 * t > 4:
            cur = N >> (4 * t); prod += R * cur; by_y += 16 * (cur + R * (cur >> 4)); by_b += 16 * (2 * cur + R * (cur >> 4)); R = int(100 / (1 + 3 * t)); t += 1
        for k, b in (("k_whir_ood_y", by_y), ("k_whir_ood_beta", by_b)):
            ms = rep.get(k, (0.0, 0))[0]
            e[k] = dict(ms=ms, launches=int(rep.get(k, (0.0, 0))[1]), products=prod, products_per_s=prod / (1e-3 * ms) if ms else None, bytes=b,
                        bytes_per_s=b / (1e-3 * ms) if ms else None)
        e["bracketed_kernel_ms"] = {k: v[0] for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])[:8]}
        res["WH_2e%d" % logN] = e
        for b in (d, com, lv):
            b.free()
    return res

# BB  the Braking base baseline (include/hobbit_brakingbase.h; test_PC option 5) at (log2 N, K) = (26, 64), (26, 128), (28, 256): commit
#     between device events and the host-returning open by wall time with its six stage times (median of `reps` after one warm-up), and in
#     the same process hobbit_brakedown_commit + _open and Our_PC's commit_standard + open_standard at the same N.  The commit runs
#     Brakedown's kernels at another shape: its per-launch times (the library's event brackets, one extra step) stand next to Brakedown's.
#     Stage 0 encodes ONE codeword of n = trs: the rows-innermost encode at rows = 1 (what the opening uses) against hobbit_encode_batch at
#     batch 1 on the same message.  "parity_commit_ms": stage 2's commit on its own, host-built and device-built lists.
#     `python scripts/bench_configs.py brakingbase [logN:K ...]` runs this entry alone.
def brakingbase_entry(shapes=((26, 64), (26, 128), (28, 256)), reps=3):
    import ctypes
    res = {}
    med = lambda v: float(np.median(v))
    def ev(fn):
        hb.timer_begin(); r = fn(); return r, hb.timer_end_ms()
    def wall(fn):
        hb.sync(); t0 = time.perf_counter(); r = fn(); return r, 1e3 * (time.perf_counter() - t0)
    def prof(fn):
        hb.profile(True); hb.profile_reset(); fn(); rep = hb.profile_report(); hb.profile(False); hb.profile_reset()
        return {k: dict(ms=round(v[0], 3), launches=int(v[1])) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])}
    for logN, K in shapes:
        N = 1 << logN; trs = mod.Hobbit.brakingbase_shape(N, K)
        d = hb.fill_splitmix(N, 1000); x = splitmix_field(logN, 8)
        e = dict(N=N, K=K, trs=trs)
        # ---- Braking base
        hb.rng_reset(); t0 = time.perf_counter(); hb.expander_init_store(trs); e["graphs_host_draw_s"] = time.perf_counter() - t0
        e["parity_commit_ms"] = parity_builders(trs)                                                                      # stage 2 alone, both builders
        c = hb.brakingbase_commit((d, N), K); g = c.open(x); assert g["checks"].tolist() == [1, 1]; c.free()          # warm: plans, workspaces, tables
        tc, to, st = [], [], []
        for _ in range(reps):
            c, t = ev(lambda: hb.brakingbase_commit((d, N), K)); tc.append(t)
            g, t = wall(lambda: c.open(x)); to.append(t); st.append(g["stage_ms"].tolist())
            assert g["checks"].tolist() == [1, 1]
            root = bytes(c.root()).hex(); c.free()
        e["brakingbase"] = dict(commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to, root=root, ps_KB=g["ps"],
                                stage_ms=dict(zip(("aggregate_encode_Cc", "replies_paths", "commit_parity_matrix", "prove_linear_code", "open_parity_matrix", "shockwave_prove_Cc"),
                                                  np.median(np.array(st), axis=0).tolist())))
        e["brakingbase"]["commit_kernels"] = prof(lambda: hb.brakingbase_commit((d, N), K).free())
        src1, dst1 = hb.fill_splitmix(trs, 5), hb.alloc(32 * trs)
        one = dict(interleaved_rows1=lambda: hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, ctypes.c_void_p(src1.ptr), ctypes.c_void_p(dst1.ptr), ctypes.c_longlong(trs), ctypes.c_uint32(1))),
                   encode_batch_1=lambda: hb._chk(hb.lib.hobbit_encode_batch(hb.ctx, ctypes.c_void_p(src1.ptr), ctypes.c_void_p(dst1.ptr), ctypes.c_longlong(trs), ctypes.c_size_t(1),
                                                                             ctypes.c_size_t(trs), ctypes.c_size_t(2 * trs))))
        e["encode_one_codeword_ms"] = {}
        for name, fn in one.items():
            try:
                fn(); hb.sync()
                e["encode_one_codeword_ms"][name] = med([ev(fn)[1] for _ in range(5)])
            except mod.HobbitError as err:
                e["encode_one_codeword_ms"][name] = "refused: %s" % err
        src1.free(); dst1.free()
        # ---- Brakedown at the same N
        B, rows = mod.Hobbit.brakedown_shape(N)
        hb.rng_reset(); hb.expander_init_store(B)
        rng = np.random.default_rng(logN)
        r = np.zeros((rows, 2), np.uint64); r[:, 0] = rng.integers(0, 1 << 31, rows); I = rng.integers(0, 2 * B, 2900).astype(np.uint64)
        c = hb.brakedown_commit((d, N)); hb.brakedown_open(c, x, r, I); c.free()
        tc, to = [], []
        for _ in range(reps):
            c, t = ev(lambda: hb.brakedown_commit((d, N))); tc.append(t)
            _, t = wall(lambda: hb.brakedown_open(c, x, r, I)); to.append(t); c.free()
        e["brakedown"] = dict(B=B, rows=rows, commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to)
        e["brakedown"]["commit_kernels"] = prof(lambda: hb.brakedown_commit((d, N)).free())
        e["commit_time_per_encoded_element_over_brakedowns"] = e["brakingbase"]["commit_ms"] / e["brakedown"]["commit_ms"]        # 2 N elements both
        # ---- Our_PC at the same N (bench.py's shape: K = 32, trs = N / (K 2^11), 5900 queries)
        Kh = 32; th = N // (Kh << 11)
        hb.rng_reset(); hb.expander_init_store(th)
        c = hb.commit_standard((d, N), Kh, th, 1); hb.open_standard((d, N), c, x, 5900, want_paths=False); c.free()
        tc, to = [], []
        for _ in range(reps):
            c, t = ev(lambda: hb.commit_standard((d, N), Kh, th, 1)); tc.append(t)
            _, t = wall(lambda: hb.open_standard((d, N), c, x, 5900, want_paths=False)); to.append(t); c.free()
        e["our_pc"] = dict(K=Kh, trs=th, commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to)
        res["BB_2e%d_K%d" % (logN, K)] = e
        d.free()
    return res

if len(sys.argv) > 1 and sys.argv[1] == "brakingbase":
    print(json.dumps(brakingbase_entry(tuple(tuple(int(v) for v in a.split(":")) for a in sys.argv[2:]) or ((26, 64), (26, 128), (28, 256)))))
    hb.close(); sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] in ("whir", "whir-bare"):
    print(json.dumps(whir_entry(tuple(int(a) for a in sys.argv[2:]) or (20, 22, 24, 26), bare=sys.argv[1] == "whir-bare")))
    hb.close(); sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] in ("parity", "parity-gather"):
    print(json.dumps(parity_entry(tuple(int(a) for a in sys.argv[2:]) or (4096, 1 << 17, 1 << 20), bare=sys.argv[1] == "parity-gather")))
    hb.close(); sys.exit(0)

# C2
n = 1 << 24
d1 = hb.fill_splitmix(n, 1); d2 = hb.precompute_beta(splitmix_field(24, 9), keep_on_device=True)
pr = np.array([33, 0], np.uint64)
out["C2_sumcheck2_2e24_ms"] = 1e3 * timed(lambda: hb.generate_2product_sumcheck_proof((d1, n), (d2, n), pr), reps=5)
del d1, d2

# C3
N, K = 1 << 26, 32; trs = N // (K << 11)
d = hb.fill_splitmix(N, 2); hb.rng_reset(); hb.expander_init_store(trs)
def c3():
    c = hb.commit_standard((d, N), K, trs, 1); c.free()
out["C3_commit_2e26_ms"] = 1e3 * timed(c3, reps=5)
del d

# Our_PC, linear_time == false (test_PC option 1: RS x RS, tensor_row_size = 128, 790 queries) at 2^26 and 2^28
for logN1 in (26, 28):
    N1 = 1 << logN1
    d = hb.fill_splitmix(N1, 4); x1 = splitmix_field(logN1, 8)
    def o1_commit():
        c = hb.commit_standard((d, N1), 32, 128, 0); c.free()
    out["O1_commit_rsrs_2e%d_ms" % logN1] = 1e3 * timed(o1_commit, reps=3)
    c1 = hb.commit_standard((d, N1), 32, 128, 0)
    def o1_open():
        r = hb.open_standard_rs((d, N1), c1, x1, 790)
        assert r["checks"].tolist() == [1, 1]
    out["O1_open_rsrs_2e%d_ms" % logN1] = 1e3 * timed(o1_open, reps=3)
    c1.free(); del d

# gate consistency with lookup gates (prove_gate_consistency_lookups) at config 4's trace shape
g = np.random.default_rng(2); circ_l = 1 << 20; Bl = 1 << 18; z = np.zeros(circ_l, np.uint64)
Sl = g.integers(0, 3, circ_l).astype(np.int32); Ll = g.integers(0, 1 << 30, circ_l).astype(np.uint64); Rl = g.integers(0, 1 << 30, circ_l).astype(np.uint64)
P61 = np.uint64((1 << 61) - 1)
Ol = np.stack([np.where(Sl == 0, Ll + Rl, np.where(Sl == 1, (Ll * Rl) % P61, g.integers(0, 1 << 60, circ_l).astype(np.uint64))), z], 1)
tsrc_l = hb.trace_source(np.stack([Ll, z], 1), np.stack([Rl, z], 1), Ol, Sl, Bl)
rl = splitmix_field(20, 3); lrand = splitmix_field(2, 77)
def gate_lk():
    r = hb.gate_consistency_lookups_stream(tsrc_l, circ_l // Bl, Bl, rl, lrand)
    assert r["checks"].tolist() == [1] * 5
out["gate_consistency_lookups_2e20_s"] = timed(gate_lk, reps=3)
del tsrc_l

# C4: math phases of the MLP prover (reference on one Xeon core: commit 5.08 s, mul-tree 5.53 s, gate 0.80 s, open 2.84 s)
import ctypes
B4 = 1 << 18; circ = 1 << 20
chunk_w = hb.to_device(hb.read_stream_PC(B4))
# (the tree stays in HBM, as in bench.py's Our_PC step; reading all of it back as the reference's host-side MT_hashes is timed separately)
out["C4_commit_witness_4x2e20_s"] = timed(lambda: hb.elastic_commit(4 * circ, B4, 1, chunk=chunk_w, levels="device"), reps=5)
out["C4_commit_witness_with_tree_readback_s"] = timed(lambda: hb.elastic_commit(4 * circ, B4, 1, chunk=chunk_w), reps=3)
lv_host, lv_dev = hb.elastic_commit(4 * circ, B4, 1, chunk=chunk_w, keep_levels=True)
src4 = hb.chunk_source(0)
pr32 = np.array([32, 0], np.uint64); px3 = splitmix_field(3, 9)
def c4_mul():
    r = hb.mul_tree_stream_shallow(src4, 8 * circ, B4, 8, circ, pr32, 5, px3, naive=False)
    assert all(st["checks"].tolist() == [1, 1, 1] for st in r["steps"]) and len(r["steps"]) == 4
out["C4_mul_tree_stream_8x2e20_s"] = timed(c4_mul, reps=3)
g = np.random.default_rng(1); z = np.zeros(circ, np.uint64)
sel = g.integers(0, 2, circ).astype(np.uint64); Lr = g.integers(0, 1 << 30, circ).astype(np.uint64); Rr = g.integers(0, 1 << 30, circ).astype(np.uint64)
P61 = np.uint64((1 << 61) - 1)
O = np.stack([np.where(sel == 1, Lr + Rr, (Lr * Rr) % P61), z], 1)
tsrc = hb.trace_source(np.stack([Lr, z], 1), np.stack([Rr, z], 1), O, sel.astype(np.int32), B4)
rg = splitmix_field(20, 3)
def c4_gate():
    r = hb.gate_consistency_stream(tsrc, circ // B4, B4, rg)
    assert r["checks"].tolist() == [1, 1, 1]
out["C4_gate_consistency_2e20_s"] = timed(c4_gate, reps=3)
chunk_r = hb.to_device(hb.read_stream(B4)); x4 = splitmix_field(22, 4)
def c4_open():
    r = hb.elastic_open(4 * circ, B4, x4, 700, commit_levels=lv_dev, chunk=chunk_r)
    assert r["checks"].tolist() == [1, 1]
out["C4_open_witness_s"] = timed(c4_open, reps=3)
out["C4_math_phases_total_s"] = sum(out[k] for k in ("C4_commit_witness_4x2e20_s", "C4_mul_tree_stream_8x2e20_s", "C4_gate_consistency_2e20_s", "C4_open_witness_s"))
out["C4_reference_one_core_s"] = {"commit": 5.08, "mul_tree": 5.53, "gate": 0.80, "open": 2.84, "note": "SURVEY.md 6; includes 2.4-2.8 s of stream generation"}
del chunk_w, lv_dev, chunk_r

# C5 (one GPU)
chunk = hb.to_device(hb.read_stream_PC(1 << 20))          # the host-side stream generator is not part of the path
for opt in (1, 2):
    hb.rng_reset()
    t = timed(lambda: hb.elastic_commit(1 << 30, 1 << 20, opt, chunk=chunk, levels="device"), reps=2, warm=1)
    out["C5_elastic_commit_2e30_B2e20_opt%d_s" % opt] = t
    if opt == 1:
        out["C5_elastic_commit_2e30_opt1_with_tree_readback_s"] = timed(lambda: hb.elastic_commit(1 << 30, 1 << 20, opt, chunk=chunk), reps=2, warm=0)
# C5 open (option 1): N = 2^26 and 2^30 with B = 2^20 (1024 chunks x 2 passes at 2^30)
chunk_r = hb.to_device(hb.read_stream(1 << 20))
for logN in (26, 30):
    N5 = 1 << logN
    lvh, lvd = hb.elastic_commit(N5, 1 << 20, 1, chunk=chunk, keep_levels=True)
    x5 = splitmix_field(logN, 6)
    def c5_open():
        r = hb.elastic_open(N5, 1 << 20, x5, 700, commit_levels=lvd, chunk=chunk_r)
        assert r["checks"].tolist() == [1, 1]
    out["C5_elastic_open_2e%d_B2e20_opt1_s" % logN] = timed(c5_open, reps=2, warm=1)
    del lvd
# C5 open (option 2, RS x expander: test_OurPC.sh's `./pigeon N 20 2`): 5900 queries, aux_commit, recursive_prover_Spielman_stream
for logN in (26, 30):
    N5 = 1 << logN
    hb.rng_reset()
    lvh, lvd = hb.elastic_commit(N5, 1 << 20, 2, chunk=chunk, keep_levels=True)      # (draws and uploads the graphs for trs = 64)
    x5 = splitmix_field(logN, 6)
    rs = hb.to_device(hb.read_stream(1 << 20))
    def c5_open2():
        r = hb.elastic_open2(N5, 1 << 20, x5, 5900, commit_levels=lvd, chunks=lambda i: rs)
        assert r["checks"].tolist() == [1]
    out["C5_elastic_open_2e%d_B2e20_opt2_s" % logN] = timed(c5_open2, reps=2, warm=1)
    del lvd
out.update(parity_entry())
out.update(whir_entry())
out.update(brakingbase_entry())
print(json.dumps(out))
hb.close()
