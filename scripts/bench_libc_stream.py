"""The libc stream on the device against the host loops (include/hobbit_libcgen.h): the measurements behind DESIGN.md section 4 "The libc stream
on the device" and profiles/libc_stream.json.

  python scripts/bench_libc_stream.py [--out FILE] [--big]

* generate_randomness(n): hobbit_generate_randomness into host memory against hobbit_generate_randomness_dev (the fill alone, and with the
  copy to host memory that the C++ mirror adds).
* the C++ mirror's generate_randomness and expander_init_store at a ladder of sizes, by the loops and by the device whatever the size
  (hobbit_host_time_libc_stream): the two switch-over sizes.  expander_init_store includes what the mirror does around the draws: the
  finalize, and _C / D filled for the host code that reads them.
* --big: also 2^28 elements and the graphs of 2^20 and 2^21.
Wall times are the best of `reps` runs after one warm-up of the path; every run starts from srandom(1).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (before the library: tests/conftest.py)
from __graft_entry__ import load_package, PKG  # noqa: E402

V = ctypes.c_void_p
libc = ctypes.CDLL(None)


def best(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); f(); ts.append(time.perf_counter() - t)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--big", action="store_true")
    a = ap.parse_args()
    mod = load_package()
    hb = mod.Hobbit(0)
    res = {"abi_generate_randomness": [], "mirror_generate_randomness": [], "mirror_expander_init_store": [], "abi_graph_draw": []}

    for lg in [16, 20, 24] + ([28] if a.big else []):
        n = 1 << lg
        host = np.empty((n, 2), np.uint64)
        dev = hb.alloc(16 * n)

        def host_loop():
            libc.srandom(1); hb.lib.hobbit_generate_randomness(ctypes.c_size_t(n), host.ctypes.data_as(V))

        def dev_fill():
            libc.srandom(1); hb._chk(hb.lib.hobbit_generate_randomness_dev(hb.ctx, ctypes.c_size_t(n), V(dev.ptr))); hb.sync()

        def dev_fill_copy():
            dev_fill(); hb._chk(hb.lib.hobbit_memcpy_d2h(hb.ctx, host.ctypes.data_as(V), V(dev.ptr), ctypes.c_size_t(16 * n)))

        reps = 2 if lg >= 28 else 5
        row = {"log2_n": lg, "host_loop_ms": 1e3 * best(host_loop, reps), "device_fill_ms": 1e3 * best(dev_fill, reps), "device_fill_and_copy_ms": 1e3 * best(dev_fill_copy, reps)}
        res["abi_generate_randomness"].append(row); print(json.dumps(row), flush=True)
        dev.free(); del host

    host_lib = ctypes.CDLL(os.path.join(PKG, "libhobbit_host.so"))
    host_lib.hobbit_host_time_libc_stream.restype = ctypes.c_double
    host_lib.hobbit_host_time_libc_stream.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int]

    def mirror(what, n, device, reps):
        host_lib.hobbit_host_time_libc_stream(what, n, device)
        return 1e3 * min(host_lib.hobbit_host_time_libc_stream(what, n, device) for _ in range(reps))

    for lg in list(range(10, 21)) + ([28] if a.big else []):
        reps = 1 if lg >= 28 else 7
        row = {"log2_n": lg, "loops_ms": mirror(0, 1 << lg, 0, reps), "device_ms": mirror(0, 1 << lg, 1, reps)}
        res["mirror_generate_randomness"].append(row); print(json.dumps(row), flush=True)
    for lg in list(range(7, 17)) + ([20, 21] if a.big else []):
        reps = 1 if lg >= 20 else 5
        row = {"log2_n": lg, "loops_ms": mirror(1, 1 << lg, 0, reps), "device_ms": mirror(1, 1 << lg, 1, reps)}
        res["mirror_expander_init_store"].append(row); print(json.dumps(row), flush=True)
    host_lib.hobbit_host_close()

    for lg in [11, 12, 13, 16] + ([20, 21] if a.big else []):
        def draw():
            libc.srandom(1); hb.graph_draw(1 << lg)
        def finalize():                                   # the part of graph_draw that is hobbit_graph_finalize (host planners + table uploads)
            ln = ctypes.c_longlong(); hb._chk(hb.lib.hobbit_graph_finalize(hb.ctx, ctypes.c_longlong(1 << lg), ctypes.byref(ln)))
        reps = 1 if lg >= 20 else 5
        row = {"log2_n": lg, "graph_draw_ms": 1e3 * best(draw, reps), "of_which_finalize_ms": 1e3 * best(finalize, reps)}
        res["abi_graph_draw"].append(row); print(json.dumps(row), flush=True)
    hb.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
