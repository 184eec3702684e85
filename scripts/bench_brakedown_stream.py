"""scripts/bench_brakedown_stream.py -- the streaming Brakedown baseline (test_Elastic_PC(2^n, 3), reference src/Elastic_PC.cpp:112-172,
561-623) on one MI355X: the prover is handed the polynomial as a stream of B-element chunks and keeps one group of four on the device.

The chunk is resident on the device and every push reads it, so the host's stream generator (read_stream_PC, sequential on the host) and
the uploads are outside the timing.  HIP events on the context's stream, median over --steps after --warmup runs.

Reported:
  commit_ms / open_ms          begin, `chunks` pushes, finish | open_begin, `chunks` aggregate pushes, `chunks` reply pushes, open_finish
                               (2935 queries; host read-back included)
  kernels_ms / launches        one extra commit + open with every launch bracketed; launches_per_group for the commit
  launch_and_tail_share        1 - (bracketed kernel time of the commit) / commit_ms.  Bracketing adds to every launch, so with back-to-back
                               kernels this comes out negative: the gaps are read from a rocprofv3 kernel trace instead
  group_encode                 one group's encode (hobbit_encode_interleaved, n = B, rows = 4: the call the pushes make), timed in two
                               separate series so that their difference is the spread of a repeated run
  elastic (--compare)          Elastic_PC options 1 and 2 at the same N with B = 2^20 (`./pigeon <logN> 20 <opt>`), as scripts/bench_configs.py
                               times them (C5): streaming commit (tree left on the device) and open, chunks resident on the device
Prints one JSON line.

usage: python scripts/bench_brakedown_stream.py [--logn 28] [--steps 5] [--warmup 2] [--compare]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUERIES = 2935


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compare", action="store_true", help="also time Elastic_PC options 1 and 2 at the same N (B = 2^20)")
    args = ap.parse_args()
    from __graft_entry__ import load_package
    mod = load_package()
    hb = mod.Hobbit(0)
    N = 1 << args.logn
    B, chunks = mod.Hobbit.brakedown_stream_shape(N)
    d_chunk = hb.fill_splitmix(B, 1000)
    rng = np.random.default_rng(args.logn)
    P = (1 << 61) - 1
    x = np.stack([rng.integers(0, P, args.logn, dtype=np.uint64), rng.integers(0, P, args.logn, dtype=np.uint64)], axis=1)
    r0 = np.array([rng.integers(0, P), rng.integers(0, P)], np.uint64)
    I = rng.integers(0, 2 * B, QUERIES).astype(np.uint64)
    out = {"workload": "streaming Brakedown test_Elastic_PC(2^%d, 3)" % args.logn, "N": N, "B": B, "chunks": chunks, "groups": chunks // 4}
    hb.rng_reset()
    hb.expander_init_store(B)
    stream = [d_chunk] * chunks

    def step():
        hb.timer_begin()
        lv = hb.brakedown_stream_commit(stream, B, levels="device")
        t_c = hb.timer_end_ms()
        hb.timer_begin()
        hb.brakedown_stream_open(stream, stream, B, chunks, x, r0, I, levels=lv)
        t_o = hb.timer_end_ms()
        root = bytes(hb.to_host(lv, (32,), np.uint8, offset=32 * (4 * B - 2))).hex()
        lv.free()
        return t_c, t_o, root

    for _ in range(args.warmup):
        step()
    tc, to = [], []
    for _ in range(args.steps):
        a, b, root = step()
        tc.append(a); to.append(b)
    out.update(commit_ms=med(tc), open_ms=med(to), total_ms=round(med(tc) + med(to), 3), root=root)
    hb.profile(1); hb.profile_reset()
    lv = hb.brakedown_stream_commit(stream, B, levels="device")
    prof_c = hb.profile_report()
    hb.profile_reset()
    hb.brakedown_stream_open(stream, stream, B, chunks, x, r0, I, levels=lv)
    prof_o = hb.profile_report()
    hb.profile(0); lv.free()
    out["commit_kernels_ms"] = {k: round(v[0], 3) for k, v in sorted(prof_c.items())}
    out["commit_launches"] = {k: int(v[1]) for k, v in sorted(prof_c.items())}
    out["open_kernels_ms"] = {k: round(v[0], 3) for k, v in sorted(prof_o.items())}
    out["open_launches"] = {k: int(v[1]) for k, v in sorted(prof_o.items())}
    out["launches_per_group"] = round(sum(int(v[1]) for v in prof_c.values()) / (chunks // 4), 2)
    ksum = sum(v[0] for v in prof_c.values())
    out["commit_kernel_sum_ms"] = round(ksum, 3)
    out["launch_and_tail_share"] = round(1.0 - ksum / out["commit_ms"], 3)

    # ---- one group's encode: the call the pushes make, two series of the same thing (their difference is the spread)
    d_mat = hb.alloc(8 * B * 16)
    hb._chk(hb.lib.hobbit_memset(hb.ctx, ctypes.c_void_p(d_mat.ptr), 0, ctypes.c_size_t(8 * B * 16)))
    reps = 8

    def enc_series():
        t = []
        for _ in range(args.warmup):
            hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, ctypes.c_void_p(d_mat.ptr), ctypes.c_void_p(d_mat.ptr), ctypes.c_longlong(B), ctypes.c_uint32(4)))
        hb.sync()
        for _ in range(args.steps):
            hb.timer_begin()
            for _ in range(reps):
                hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, ctypes.c_void_p(d_mat.ptr), ctypes.c_void_p(d_mat.ptr), ctypes.c_longlong(B), ctypes.c_uint32(4)))
            t.append(hb.timer_end_ms() / reps)
        return med(t)

    a, b = enc_series(), enc_series()
    out["group_encode"] = {"series_a_ms": a, "series_b_ms": b, "spread_ms": round(abs(a - b), 3), "per_commit_ms": round(min(a, b) * (chunks // 4), 3)}
    d_mat.free()

    if args.compare:
        # HOBBIT's own streaming PCS at the same N, the calls of scripts/bench_configs.py (C5); the reference's default streams repeat one chunk
        Be = 1 << 20
        splitmix_field = mod.splitmix_field
        chunk = hb.to_device(hb.read_stream_PC(Be)); chunk_r = hb.to_device(hb.read_stream(Be))
        xe = splitmix_field(args.logn, 6)
        el = {"B": Be, "chunks": N // Be}

        def series(fn):
            for _ in range(args.warmup):
                fn()
            t = []
            for _ in range(args.steps):
                hb.timer_begin(); fn(); t.append(hb.timer_end_ms())
            return med(t)

        for opt in (1, 2):
            hb.rng_reset()
            el["opt%d_commit_ms" % opt] = series(lambda: hb.elastic_commit(N, Be, opt, chunk=chunk, levels="device"))
            hb.rng_reset()
            lvh, lvd = hb.elastic_commit(N, Be, opt, chunk=chunk, keep_levels=True)
            if opt == 1:
                def op():
                    r = hb.elastic_open(N, Be, xe, 700, commit_levels=lvd, chunk=chunk_r)
                    assert r["checks"].tolist() == [1, 1]
            else:
                def op():
                    r = hb.elastic_open2(N, Be, xe, 5900, commit_levels=lvd, chunks=lambda i: chunk_r)
                    assert r["checks"].tolist() == [1]
            el["opt%d_open_ms" % opt] = series(op)
            el["opt%d_total_ms" % opt] = round(el["opt%d_commit_ms" % opt] + el["opt%d_open_ms" % opt], 3)
            del lvd, lvh
        out["elastic"] = el
    hb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
