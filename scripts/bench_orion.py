"""scripts/bench_orion.py -- measurements behind the Orion baseline (include/hobbit_orion.h); prints one JSON object.

  python scripts/bench_orion.py encode <logN>     the column pass of the commitment at N = 2^logN on one 2B x 2B buffer, in place, between
                                                  device events: hobbit_encode_interleaved at rows = 2B (every column, k_enc_ilv's order)
                                                  against hobbit_encode_interleaved_ld over the first `len` columns in the plain order
                                                  (strip 0) and strip-major at 64, 128 and 256 columns, and over all 2B columns in the plain
                                                  order (the order alone, without the width cut).  One warm-up of every variant, then ROUNDS
                                                  rounds, the order of the variants reversed every other round.  The in-place encode reads
                                                  rows [0, B) and writes the others, so every run does the same work on the same bytes.
  python scripts/bench_orion.py baseline <logN>   commit (device events) and open (host wall time: it returns synchronised) with the six stage
                                                  times and the proof size, medians of REPS after one warm-up; in the same process Brakedown,
                                                  Braking base (K = max(128, N / 2^20)) and Our_PC (K = 32, 5900 queries) at the same N.
One process per shape: the 2^28 tensor, its tree and the 2^24 opening paths are 16 + 16 + 15 GB.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

ROUNDS, REPS = 6, 3
V, S, L, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_uint32
mod = load_package()


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), runs=[round(float(t), 4) for t in v])


def encode(hb, logN):
    N = 1 << logN; B, _ = mod.Hobbit.orion_shape(N); W = 2 * B
    hb.rng_reset(); ln = hb.expander_init_store(B)
    mat = hb.fill_splitmix(W * W, 2828)
    ilv = lambda: hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, V(mat.ptr), V(mat.ptr), L(B), U32(W)))  # noqa: E731
    ld = lambda width, strip: (lambda: hb._chk(hb.lib.hobbit_encode_interleaved_ld_order(hb.ctx, V(mat.ptr), L(B), S(width), S(W), U32(strip))))  # noqa: E731
    variants = [("interleaved_rows_2B", ilv), ("ld_all_columns_plain", ld(W, 0)), ("ld_len_plain", ld(ln, 0)), ("ld_len_strip64", ld(ln, 64)),
                ("ld_len_strip128", ld(ln, 128)), ("ld_len_strip256", ld(ln, 256))]
    for _, fn in variants:
        fn()
    hb.sync()
    times = {k: [] for k, _ in variants}
    for rnd in range(ROUNDS):
        for k, fn in (variants if rnd % 2 == 0 else variants[::-1]):
            hb.timer_begin(); fn(); times[k].append(hb.timer_end_ms())
    return dict(N=N, B=B, len=ln, columns_encoded_fraction=ln / W, rounds=ROUNDS, ms={k: stat(v) for k, v in times.items()})


def baseline(hb, logN):
    from oracle.pyoracle import splitmix_field
    N = 1 << logN; B, Q = mod.Hobbit.orion_shape(N)
    d = hb.fill_splitmix(N, 1000); x = splitmix_field(logN, 8)
    med = lambda v: float(np.median(v))  # noqa: E731

    def ev(fn):
        hb.timer_begin(); r = fn(); return r, hb.timer_end_ms()

    def wall(fn):
        hb.sync(); t0 = time.perf_counter(); r = fn(); return r, 1e3 * (time.perf_counter() - t0)

    def prof(fn):
        hb.profile(True); hb.profile_reset(); fn(); hb.sync(); rep = hb.profile_report(); hb.profile(False); hb.profile_reset()
        return {k: dict(ms=round(v[0], 3), launches=int(v[1])) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])[:10]}
    e = dict(N=N, B=B, Q=Q)
    # ---- Orion
    hb.rng_reset(); t0 = time.perf_counter(); hb.expander_init_store(B); e["graphs_host_draw_s"] = time.perf_counter() - t0
    try:
        c = hb.orion_commit((d, N)); g = c.open(x, want_ps=False); assert g["checks"].tolist() == [1, 1]; g["paths"].free(); c.free()   # warm
        tc, to, st = [], [], []
        for _ in range(REPS):
            c, t = ev(lambda: hb.orion_commit((d, N))); tc.append(t)
            g, t = wall(lambda: c.open(x, want_ps=False)); to.append(t); st.append(g["stage_ms"].tolist())
            assert g["checks"].tolist() == [1, 1]
            g["paths"].free(); root = bytes(c.root()).hex(); c.free()
        # the proof size is accounting outside the opening: the same opening without and with it, no paths produced
        c = hb.orion_commit((d, N))
        _, t_open = wall(lambda: c.open(x, want_paths=False, want_ps=False)); g, t_both = wall(lambda: c.open(x, want_paths=False, want_ps=True)); c.free()
        e["orion"] = dict(commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to, root=root, ps_KB=g["ps"], paths_bytes=Q * Q * logN * 32,
                          open_without_paths_ms=t_open, proof_size_call_ms=t_both - t_open,
                          stage_ms=dict(zip(("gather_C", "commit_parity_matrix", "prove_linear_code_batch", "open_parity_matrix", "shockwave_prove_C", "grid_paths"),
                                            np.median(np.array(st), axis=0).tolist())))
        e["orion"]["commit_kernels"] = prof(lambda: hb.orion_commit((d, N)).free())
    except mod.HobbitError as err:
        e["orion"] = "refused: %s" % err
    # ---- Brakedown at the same N
    Bd, rows = mod.Hobbit.brakedown_shape(N)
    hb.rng_reset(); hb.expander_init_store(Bd)
    rng = np.random.default_rng(logN)
    r = np.zeros((rows, 2), np.uint64); r[:, 0] = rng.integers(0, 1 << 31, rows); I = rng.integers(0, 2 * Bd, 2900).astype(np.uint64)
    c = hb.brakedown_commit((d, N)); hb.brakedown_open(c, x, r, I); c.free()
    tc, to = [], []
    for _ in range(REPS):
        c, t = ev(lambda: hb.brakedown_commit((d, N))); tc.append(t)
        _, t = wall(lambda: hb.brakedown_open(c, x, r, I)); to.append(t); c.free()
    e["brakedown"] = dict(B=Bd, rows=rows, commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to)
    # ---- Braking base at the same N
    K = max(128, N >> 20); trs = mod.Hobbit.brakingbase_shape(N, K)
    hb.rng_reset(); hb.expander_init_store(trs)
    c = hb.brakingbase_commit((d, N), K); g = c.open(x); c.free()
    tc, to = [], []
    for _ in range(REPS):
        c, t = ev(lambda: hb.brakingbase_commit((d, N), K)); tc.append(t)
        g, t = wall(lambda: c.open(x)); to.append(t); c.free()
    e["brakingbase"] = dict(K=K, trs=trs, commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to, ps_KB=g["ps"])
    # ---- Our_PC at the same N (bench.py's shape: K = 32, trs = N / (K 2^11), 5900 queries)
    Kh = 32; th = N // (Kh << 11)
    hb.rng_reset(); hb.expander_init_store(th)
    c = hb.commit_standard((d, N), Kh, th, 1); hb.open_standard((d, N), c, x, 5900, want_paths=False); c.free()
    tc, to = [], []
    for _ in range(REPS):
        c, t = ev(lambda: hb.commit_standard((d, N), Kh, th, 1)); tc.append(t)
        _, t = wall(lambda: hb.open_standard((d, N), c, x, 5900, want_paths=False)); to.append(t); c.free()
    e["our_pc"] = dict(K=Kh, trs=th, commit_ms=med(tc), open_ms=med(to), commit_runs=tc, open_runs=to)
    return e


def main():
    what, logN = sys.argv[1], int(sys.argv[2])
    hb = mod.Hobbit(0)
    try:
        print(json.dumps({"%s_2e%d" % (what, logN): (encode if what == "encode" else baseline)(hb, logN)}))
    finally:
        hb.close()


if __name__ == "__main__":
    main()
