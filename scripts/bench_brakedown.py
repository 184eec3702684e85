"""scripts/bench_brakedown.py -- the Brakedown comparison baseline (test_PC(2^n, 3, K), reference src/Our_PC.cpp:197-236, 432-520) against
HOBBIT's own Our_PC (test_PC(2^n, 4, K): what bench.py times) at the same N, in one process on one MI355X.

Reported (HIP events on the context's stream, after warm-up; median over --steps):
  brakedown_commit_ms / brakedown_open_ms   hobbit_brakedown_commit (transpose, rows-innermost encode, column digests, tree) and
                                            hobbit_brakedown_open (aggregates, 2900 replies, paths; host read-back included)
  brakedown_kernels_ms                      one extra step with every launch bracketed
  encode                                    the rows-innermost encode of (B, rows) alone, against hobbit_encode_batch on the same messages;
                                            its edge-gather bytes per second against HBM peak (8.0 TB/s) and the 5.7-7.9 TB/s gather roof
  hobbit_commit_open_ms, ratio              commit_standard + open_standard (bench.py's step) at the same N, and hobbit / brakedown
  graph_finalize_ms                         hobbit_graph_finalize at n = B (the rows-innermost and tiled plans are built on first use)
Prints one JSON line.

usage: python scripts/bench_brakedown.py [--logn 28] [--chunks 32] [--steps 5] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0
GATHER_ROOF_TBS = (5.7, 7.9)


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--chunks", type=int, default=32, help="K of HOBBIT's commit_standard (bench.py's default)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=5900, help="HOBBIT open's queries (bench.py's default)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    mod = load_package()
    hb = mod.Hobbit(0)
    N = 1 << args.logn
    B, rows = mod.Hobbit.brakedown_shape(N)
    d_poly = hb.fill_splitmix(N, 1000)
    rng = np.random.default_rng(args.logn)
    P = (1 << 61) - 1
    x = np.stack([rng.integers(0, P, args.logn, dtype=np.uint64), rng.integers(0, P, args.logn, dtype=np.uint64)], axis=1)
    r = np.zeros((rows, 2), np.uint64); r[:, 0] = rng.integers(0, 1 << 31, rows)
    I = rng.integers(0, 2 * B, 2900).astype(np.uint64)
    out = {"workload": "Brakedown test_PC(2^%d, 3, .) vs HOBBIT test_PC(2^%d, 4, %d)" % (args.logn, args.logn, args.chunks), "N": N, "B": B, "rows": rows}

    # ---- Brakedown
    hb.rng_reset()
    code_len = hb.expander_init_store(B)           # the row code's graphs (libc draws, reference order)
    edges = sum(int(L) * int(d) for (L, R, d, nbr, w) in hb._graph_levels.values())
    t0 = time.perf_counter()
    hb._chk(hb.lib.hobbit_graph_finalize(hb.ctx, ctypes.c_longlong(B), None))      # what a context pays before its first Brakedown commit
    out["graph_finalize_ms"] = round(1e3 * (time.perf_counter() - t0), 1)

    def bd_step():
        hb.timer_begin()
        c = hb.brakedown_commit((d_poly, N))
        t_c = hb.timer_end_ms()
        hb.timer_begin()
        hb.brakedown_open(c, x, r, I)
        t_o = hb.timer_end_ms()
        return c, t_c, t_o

    for _ in range(args.warmup):
        bd_step()[0].free()
    tc, to = [], []
    for _ in range(args.steps):
        c, a, b = bd_step()
        tc.append(a); to.append(b)
        root = bytes(c.root()).hex()
        c.free()
    out.update(brakedown_commit_ms=med(tc), brakedown_open_ms=med(to), brakedown_total_ms=round(med(tc) + med(to), 3), brakedown_root=root)
    hb.profile(1); hb.profile_reset()
    c, _, _ = bd_step(); c.free()
    prof = hb.profile_report()
    hb.profile(0)
    out["brakedown_kernels_ms"] = {k: round(v[0], 3) for k, v in sorted(prof.items())}
    out["brakedown_launches"] = {k: int(v[1]) for k, v in sorted(prof.items())}

    # ---- the encode alone: rows-innermost against hobbit_encode_batch on the same (B, rows) messages
    d_dst = hb.alloc(32 * N)
    lib = hb.lib

    def ilv():
        hb._chk(lib.hobbit_encode_interleaved(hb.ctx, ctypes.c_void_p(d_poly.ptr), ctypes.c_void_p(d_dst.ptr), ctypes.c_longlong(B), ctypes.c_uint32(rows)))

    def batch():
        hb._chk(lib.hobbit_encode_batch(hb.ctx, ctypes.c_void_p(d_poly.ptr), ctypes.c_void_p(d_dst.ptr), ctypes.c_longlong(B), ctypes.c_size_t(rows),
                                        ctypes.c_size_t(B), ctypes.c_size_t(2 * B)))

    enc = {}
    for name, fn in (("interleaved", ilv), ("encode_batch", batch)):
        for _ in range(args.warmup):
            fn()
        hb.sync()
        t = []
        for _ in range(args.steps):
            hb.timer_begin(); fn(); t.append(hb.timer_end_ms())
        enc[name + "_ms"] = med(t)
    gather = edges * rows * 16
    enc["edges"] = edges; enc["codeword_len"] = code_len
    enc["edge_gather_bytes"] = gather
    enc["gather_TBs"] = round(gather / (enc["interleaved_ms"] * 1e-3) / 1e12, 3)
    enc["gather_frac_of_hbm_peak"] = round(enc["gather_TBs"] / HBM_TBS, 3)
    enc["gather_frac_of_gather_roof"] = [round(enc["gather_TBs"] / g, 3) for g in GATHER_ROOF_TBS]
    enc["speedup_vs_encode_batch"] = round(enc["encode_batch_ms"] / enc["interleaved_ms"], 3)
    out["encode"] = enc
    d_dst.free()

    # ---- HOBBIT's Our_PC at the same N (bench.py's step: commit_standard queued, open_standard behind it)
    K = args.chunks
    trs = N // (K << 11)
    hb.rng_reset()
    hb.expander_init_store(trs)
    x_open = x

    def hb_step():
        hb.timer_begin()
        c = hb.commit_standard((d_poly, N), K, trs, 1, sync=False)
        hb.open_core((d_poly, N), c, x_open, args.queries, full=True)
        t = hb.timer_end_ms()
        c.free()
        return t

    for _ in range(max(args.warmup, 2)):
        hb_step()
    th = [hb_step() for _ in range(args.steps)]
    out["hobbit_commit_open_ms"] = med(th)
    out["hobbit_over_brakedown"] = round(out["hobbit_commit_open_ms"] / out["brakedown_total_ms"], 3)
    hb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
