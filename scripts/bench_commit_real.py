"""Timings of the base-field commit (include/hobbit_real.h) beside the full commit of the same polynomial widened, in ONE process on ONE build.

The polynomial is test_PC's own stream (generate_randomness from srandom(1)), the graphs are drawn for trs = N / (2048 K).  A build without
hobbit_real.h (the parent commit's) runs the full legs only, on the same polynomial drawn as F elements: its root must be the one this build
prints.  Two builds are compared by alternating processes in one GPU session (scripts/README.md); this script is one such process.

    python scripts/bench_commit_real.py [--logn 28] [--chunks 32] [--reps 6] [--host] [--label NAME]

Prints one JSON line: per leg the event-timed commits (ms), the aggregate (ms), per-kernel times of one extra profiled commit, and with --host
the wall time of the drop-in upload commits from pageable host memory (8 against 16 bytes per coefficient).
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from __graft_entry__ import load_package

c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t
ap = argparse.ArgumentParser()
ap.add_argument("--logn", type=int, default=28)
ap.add_argument("--chunks", type=int, default=32)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--host", action="store_true")
ap.add_argument("--label", default="")
a = ap.parse_args()

mod = load_package(); hb = mod.Hobbit(0)
N, K = 1 << a.logn, a.chunks
trs = N // (K << 11); M = N // K
has_real = hasattr(mod, "REAL_SYMBOLS") and hasattr(hb.lib, "hobbit_commit_standard_real")
hb.rng_reset()
if has_real:
    d_real = hb.generate_randomness_real_dev(N)
    d_wide = hb.alloc(16 * N)
    hb._chk(hb.lib.hobbit_widen_real(hb.ctx, c_vp(d_real.ptr), c_vp(d_wide.ptr), c_sz(N)))
else:
    d_real = None
    d_wide = hb.generate_randomness_dev(N)
hb.graph_draw(trs)
beta = mod.splitmix_field(K, 5)
d_aggr = hb.alloc(16 * M)

legs = {"full": lambda: hb.commit_standard((d_wide, N), K, trs, 1, sync=False)}
aggs = {"full": lambda: hb.lib.hobbit_aggregate(hb.ctx, c_vp(d_wide.ptr), c_sz(N), beta.ctypes.data_as(c_vp), K, c_vp(d_aggr.ptr))}
if has_real:
    legs["real"] = lambda: hb.commit_standard_real((d_real, N), K, trs, 1, sync=False)
    aggs["real"] = lambda: hb.lib.hobbit_aggregate_real(hb.ctx, c_vp(d_real.ptr), c_sz(N), beta.ctypes.data_as(c_vp), K, c_vp(d_aggr.ptr))

out = {"label": a.label, "logn": a.logn, "K": K, "trs": trs, "has_real": has_real, "commit_ms": {}, "aggregate_ms": {}, "kernels_ms": {}, "root": {}}
for name, fn in legs.items():                          # warm every leg once: workspaces, tables, code objects
    c = fn(); hb.sync(); out["root"][name] = c.root().tobytes().hex(); c.free()
    hb._chk(aggs[name]()); hb.sync()
for r in range(a.reps):                                # alternating
    for name, fn in legs.items():
        fn().free()                                    # untimed: the parked buffers of the other leg's size are released and this leg's parked, outside the timed commit
        hb.timer_begin(); c = fn(); ms = hb.timer_end_ms()
        out["commit_ms"].setdefault(name, []).append(round(ms, 3)); c.free()
        hb.timer_begin(); hb._chk(aggs[name]()); ms = hb.timer_end_ms()
        out["aggregate_ms"].setdefault(name, []).append(round(ms, 4))
for name, fn in legs.items():                          # one profiled commit per leg (its own run: the profiler serialises)
    hb.profile(True); hb.profile_reset()
    c = fn(); hb.sync()
    out["kernels_ms"][name] = {k: round(v[0], 3) for k, v in hb.profile_report().items() if v[0] > 0.01}
    hb.profile(False); hb.profile_reset(); c.free()
if a.host:
    hosts = {"full": (hb.to_host(d_wide, (N, 2), np.uint64), hb.commit_standard_host)}
    if has_real:
        hosts["real"] = (hb.to_host(d_real, (N,), np.uint64), hb.commit_standard_real_host)
    out["host_commit_ms"] = {}
    for name, (h, fn) in hosts.items():
        c, d = fn(h, K, trs, 1); assert c.root().tobytes().hex() == out["root"][name]; c.free(); d.free()
    for r in range(max(3, a.reps // 2)):
        for name, (h, fn) in hosts.items():
            legs[name]().free()                        # (untimed, as above: this leg's buffers parked)
            hb.sync(); t0 = time.perf_counter(); c, d = fn(h, K, trs, 1); ms = 1e3 * (time.perf_counter() - t0)      # (the binding ends with a synchronise)
            out["host_commit_ms"].setdefault(name, []).append(round(ms, 2)); c.free(); d.free()
if len(set(out["root"].values())) != 1:
    out["ERROR"] = "roots differ"
print(json.dumps(out))
hb.close()
