"""Timings of the base-field RS x RS commit (include/hobbit_real_rs.h) beside the full RS x RS commit of the same polynomial widened, in ONE process
on ONE build.

The polynomial is test_PC's own stream (generate_randomness from srandom(1)), trs = 128 as test_PC option 1 sets it.  A build without
hobbit_real_rs.h (the parent commit's) runs the full legs only, on the same polynomial: its root must be the one this build prints.  Two builds are
compared by alternating processes in one GPU session (scripts/README.md); this script is one such process.

    python scripts/bench_commit_real_rs.py [--logn 28] [--chunks 32] [--trs 128] [--reps 4] [--host] [--profile] [--label NAME]

Prints one JSON line: per leg the event-timed commits (ms) and the aggregate (ms); with --profile, INSTEAD of the timed legs, the per-kernel times
of one profiled commit per leg (a run of its own: the profiler serialises); with --host the wall time of the drop-in upload commits from pageable
host memory (8 against 16 bytes per coefficient).
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
ap.add_argument("--trs", type=int, default=128)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--host", action="store_true")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--label", default="")
a = ap.parse_args()

mod = load_package(); hb = mod.Hobbit(0)
N, K, trs = 1 << a.logn, a.chunks, a.trs
M = N // K
has_real = hasattr(mod, "REAL_RS_SYMBOLS") and hasattr(hb.lib, "hobbit_commit_standard_real_rs")
hb.rng_reset()
d_real = hb.generate_randomness_real_dev(N)
d_wide = hb.alloc(16 * N)
hb._chk(hb.lib.hobbit_widen_real(hb.ctx, c_vp(d_real.ptr), c_vp(d_wide.ptr), c_sz(N)))
beta = mod.splitmix_field(K, 5)
d_aggr = hb.alloc(16 * M)

legs = {"full": lambda: hb.commit_standard((d_wide, N), K, trs, 0, sync=False)}
aggs = {"full": lambda: hb.lib.hobbit_aggregate(hb.ctx, c_vp(d_wide.ptr), c_sz(N), beta.ctypes.data_as(c_vp), K, c_vp(d_aggr.ptr)),
        "real": lambda: hb.lib.hobbit_aggregate_real(hb.ctx, c_vp(d_real.ptr), c_sz(N), beta.ctypes.data_as(c_vp), K, c_vp(d_aggr.ptr))}
if has_real:
    legs["real"] = lambda: hb.commit_standard_real_rs((d_real, N), K, trs, sync=False)

out = {"label": a.label, "logn": a.logn, "K": K, "trs": trs, "has_real": has_real, "commit_ms": {}, "aggregate_ms": {}, "kernels_ms": {}, "root": {}}
for name, fn in legs.items():                          # warm every leg once: workspaces, tables, code objects
    c = fn(); hb.sync(); out["root"][name] = c.root().tobytes().hex(); c.free()
for name in aggs:
    hb._chk(aggs[name]()); hb.sync()
if a.profile:
    for name, fn in legs.items():                      # one profiled commit per leg
        fn().free()
        hb.profile(True); hb.profile_reset()
        c = fn(); hb.sync()
        out["kernels_ms"][name] = {k: round(v[0], 3) for k, v in hb.profile_report().items() if v[0] > 0.01}
        hb.profile(False); hb.profile_reset(); c.free()
else:
    for r in range(a.reps):                            # alternating
        for name, fn in legs.items():
            fn().free()                                # untimed: the parked buffers of the other leg's size are released and this leg's parked, outside the timed commit
            hb.timer_begin(); c = fn(); ms = hb.timer_end_ms()
            out["commit_ms"].setdefault(name, []).append(round(ms, 3)); c.free()
        for name in aggs:
            hb.timer_begin(); hb._chk(aggs[name]()); ms = hb.timer_end_ms()
            out["aggregate_ms"].setdefault(name, []).append(round(ms, 4))
if a.host:
    hosts = {"full": (hb.to_host(d_wide, (N, 2), np.uint64), lambda h: hb.commit_standard_host(h, K, trs, 0))}
    if has_real:
        hosts["real"] = (hb.to_host(d_real, (N,), np.uint64), lambda h: hb.commit_standard_real_rs_host(h, K, trs))
    out["host_commit_ms"] = {}
    for name, (h, fn) in hosts.items():
        c, d = fn(h); assert c.root().tobytes().hex() == out["root"][name]; c.free(); d.free()
    for r in range(3):
        for name, (h, fn) in hosts.items():
            legs[name]().free()                        # (untimed, as above: this leg's buffers parked)
            hb.sync(); t0 = time.perf_counter(); c, d = fn(h); ms = 1e3 * (time.perf_counter() - t0)      # (the binding ends with a synchronise)
            out["host_commit_ms"].setdefault(name, []).append(round(ms, 2)); c.free(); d.free()
if len(set(out["root"].values())) != 1:
    out["ERROR"] = "roots differ"
print(json.dumps(out))
hb.close()
