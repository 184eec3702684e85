"""Timings of the streaming commit and opening on base-field chunks (include/hobbit_elastic_real.h) beside the full forms on the same chunks
widened, in ONE process on ONE build, with the stream's (repeating) chunk resident on the device.

The chunks are the default streams of the reference: read_stream_PC's for the commit, read_stream's for the opening.  A build without
hobbit_elastic_real.h (the parent commit's) runs the full legs only: its root must be the one this build prints.  Two builds are compared by
alternating processes in one GPU session (scripts/README.md); this script is one such process.

    python scripts/bench_elastic_real.py [--logn 30] [--logb 20] [--opt 1] [--reps 3] [--open] [--label NAME]

Prints one JSON line: per leg the event-timed commits (ms; begin, N / B pushes, finish), with --open the wall time of one opening (ms), the
handle's device bytes, and the per-launch mean of every kernel of one extra profiled commit of 8 chunks (ms).
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
ap.add_argument("--logn", type=int, default=30)
ap.add_argument("--logb", type=int, default=20)
ap.add_argument("--opt", type=int, default=1)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--open", action="store_true")
ap.add_argument("--label", default="")
a = ap.parse_args()

mod = load_package(); hb = mod.Hobbit(0)
N, B = 1 << a.logn, 1 << a.logb
lin, trs = (0, B >> 11) if a.opt == 1 else (1, B >> 14)
has_real = hasattr(mod, "ELASTIC_REAL_SYMBOLS") and hasattr(hb.lib, "hobbit_elastic_push_real")


def stream_pc(n):                                      # read_stream_PC's default stream as reals (its img is 0)
    out = np.zeros(n, np.uint64); v = 322322
    for i in range(n):
        out[i] = v; v = (v * v + i) % mod.P
    return out


def widen(x):
    w = np.zeros((x.shape[0], 2), np.uint64); w[:, 0] = x
    return w


x_pc = stream_pc(B)
x_rs = np.arange(B, dtype=np.uint64) % np.uint64(1024) + np.uint64(1)
chunk = {"full": hb.to_device(widen(x_pc))}; ochunk = {"full": hb.to_device(widen(x_rs))}
if has_real:
    chunk["real"] = hb.to_device(x_pc); ochunk["real"] = hb.to_device(x_rs)
hb.rng_reset()
if lin:
    hb.graph_draw(trs)
lv = hb.alloc(32 * 8 * B)
held = {}


def commit(name, nchunks):
    e = c_vp()
    begin, push = (hb.lib.hobbit_elastic_begin_real, hb.lib.hobbit_elastic_push_real) if name == "real" else (hb.lib.hobbit_elastic_begin, hb.lib.hobbit_elastic_push)
    hb._chk(begin(hb.ctx, B, trs, lin, 1, ctypes.byref(e)))
    if has_real:
        held[name] = hb.lib.hobbit_elastic_device_bytes(e)
    for _ in range(nchunks):
        hb._chk(push(hb.ctx, e, chunk[name].ptr))
    hb._chk(hb.lib.hobbit_elastic_finish(hb.ctx, e, lv.ptr))
    hb.lib.hobbit_elastic_free(e)


def root():
    r = np.zeros(32, np.uint8)
    hb._chk(hb.lib.hobbit_memcpy_d2h(hb.ctx, r.ctypes.data, lv.ptr + 32 * (8 * B - 2), 32))
    return r.tobytes().hex()


def opening(name):
    x = mod.splitmix_field(a.logn, 7)
    ctypes.CDLL(None).srandom(99)
    real = {"_real": True} if name == "real" else {}
    if a.opt == 1:
        return hb.elastic_open(N, B, x, 700, commit_levels=lv, chunk=ochunk[name], **real)
    return hb.elastic_open2(N, B, x, 5900, commit_levels=lv, chunks=lambda i: ochunk[name], **real)


names = ["full", "real"] if has_real else ["full"]
out = {"label": a.label, "logn": a.logn, "logb": a.logb, "opt": a.opt, "trs": trs, "has_real": has_real, "commit_ms": {}, "open_wall_ms": {}, "kernels_ms_per_launch": {}, "root": {}}
for name in names:                                     # warm every leg once: workspaces, tables, code objects
    commit(name, N // B); hb.sync(); out["root"][name] = root()
for r in range(a.reps):                                # alternating
    for name in names:
        hb.sync(); hb.timer_begin(); commit(name, N // B); ms = hb.timer_end_ms()
        out["commit_ms"].setdefault(name, []).append(round(ms, 3))
if a.open:
    for name in names:
        opening(name)                                  # warm
    for r in range(a.reps):
        for name in names:
            hb.sync(); t0 = time.perf_counter(); o = opening(name); ms = 1e3 * (time.perf_counter() - t0)
            out["open_wall_ms"].setdefault(name, []).append(round(ms, 2))
            out.setdefault("open_cf_root", {})[name] = o["cf_root"].tobytes().hex()
for name in names:                                     # one profiled commit of 8 chunks per leg (its own run: the profiler serialises)
    hb.profile(True); hb.profile_reset()
    commit(name, 8); hb.sync()
    out["kernels_ms_per_launch"][name] = {k: [round(v[0] / max(v[1], 1), 4), v[1]] for k, v in hb.profile_report().items() if v[1] > 0}
    hb.profile(False); hb.profile_reset()
out["device_bytes"] = held
if len(set(out["root"].values())) != 1 or len(set(out.get("open_cf_root", {"x": 0}).values())) != 1:
    out["ERROR"] = "roots differ"
print(json.dumps(out))
hb.close()
