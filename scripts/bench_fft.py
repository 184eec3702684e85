"""scripts/bench_fft.py -- the transform at every length (hobbit_fft_batch / hobbit_fft_any), timed with HIP events on the context's stream
(hobbit_timer_*): warm-up, then the median of --steps calls; every figure is repeated --repeats times and all repeats are kept.

  forward 2^13 .. 2^24 through hobbit_fft_batch, on this build and -- with --parent <libhobbit_hip.so of the parent commit> -- on the parent
          build in the same session (a fresh process per build, alternating).  The kernels of that path are meant to be untouched, so the
          allowed difference is the parent's own min-to-max spread over its repeats; the per-kernel launch counts at 2^13, 17, 20, 22, 24 are
          recorded for both.
  inverse 2^13 .. 2^28 and forward 2^25 .. 2^28 through hobbit_fft_any, batch 1; inverse / forward per length.
  2^25 .. 2^28: sweeps over the data, sweeps * 32 B * len / time against HBM peak, and time per element and log2(len) against
          the 2^24 forward of the same session.
  the callers' shapes: batch 32 at 2^17, batch 16 at 2^23, both directions.

Writes one JSON document (--out, default profiles/fft_any_length.json) and prints a one-line summary.

usage: python scripts/bench_fft.py [--parent path/to/parent/libhobbit_hip.so] [--steps 10] [--warmup 3] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
HBM_TBS = 8.0
COUNT_AT = (13, 17, 20, 22, 24)
SWEEPS = {25: 4, 26: 4, 27: 5, 28: 5}          # transpose, (transpose,) FFT-4096, columns of the 2^17..2^20 rows, 256-point columns


class Lib:
    """the few calls this script needs, over ctypes alone: a parent build lacks symbols the package insists on"""

    def __init__(self, path):
        V, S, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib = lib = ctypes.CDLL(path)
        lib.hobbit_last_error.restype = ctypes.c_char_p
        protos = {"hobbit_ctx_create": [I, V], "hobbit_ctx_destroy": [V], "hobbit_last_error": [V], "hobbit_sync": [V], "hobbit_malloc": [V, S, V],
                  "hobbit_free": [V, V], "hobbit_timer_begin": [V], "hobbit_timer_end_ms": [V, V], "hobbit_profile_enable": [V, I],
                  "hobbit_profile_reset": [V], "hobbit_profile_get": [V, ctypes.c_char_p, V, V], "hobbit_profile_names": [V, V, S],
                  "hobbit_fill_splitmix": [V, V, S, ctypes.c_uint64], "hobbit_fft_batch": [V, V, I, S, S, I]}
        self.has_any = hasattr(lib, "hobbit_fft_any")
        if self.has_any:
            protos["hobbit_fft_any"] = [V, V, I, S, S, I]
        for name, args in protos.items():
            getattr(lib, name).argtypes = args
        self.ctx = V()
        if lib.hobbit_ctx_create(0, ctypes.byref(self.ctx)) != 0:
            raise SystemExit("no usable HIP device")

    def chk(self, rc):
        if rc != 0:
            raise SystemExit("rc=%d: %s" % (rc, self.lib.hobbit_last_error(self.ctx).decode()))

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self.chk(self.lib.hobbit_malloc(self.ctx, nbytes, ctypes.byref(p)))
        return p.value

    def fft(self, entry, ptr, logn, batch, inverse):
        self.chk(getattr(self.lib, entry)(self.ctx, ptr, logn, batch, 1 << logn, int(inverse)))

    def time_ms(self, entry, ptr, logn, batch, inverse, warmup, steps):
        for _ in range(warmup):
            self.fft(entry, ptr, logn, batch, inverse)
        self.chk(self.lib.hobbit_sync(self.ctx))
        t = []
        for _ in range(steps):
            self.chk(self.lib.hobbit_timer_begin(self.ctx))
            self.fft(entry, ptr, logn, batch, inverse)
            ms = ctypes.c_float()
            self.chk(self.lib.hobbit_timer_end_ms(self.ctx, ctypes.byref(ms)))
            t.append(ms.value)
        return statistics.median(t)

    def launch_counts(self, entry, ptr, logn, inverse):
        self.chk(self.lib.hobbit_profile_enable(self.ctx, 1)); self.chk(self.lib.hobbit_profile_reset(self.ctx))
        self.fft(entry, ptr, logn, 1, inverse)
        self.chk(self.lib.hobbit_sync(self.ctx))
        buf = ctypes.create_string_buffer(8192)
        self.chk(self.lib.hobbit_profile_names(self.ctx, buf, 8192))
        out = {}
        for name in [s for s in buf.value.decode().split(";") if s]:
            ms = ctypes.c_double(); cnt = ctypes.c_longlong()
            self.chk(self.lib.hobbit_profile_get(self.ctx, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
            if cnt.value:
                out[name] = cnt.value
        self.chk(self.lib.hobbit_profile_enable(self.ctx, 0))
        return out


def worker(args):
    L = Lib(args.lib)
    top = 28 if (L.has_any and not args.forward_only) else 24
    n = max(1 << top, 32 << 17, 16 << 23)
    buf = L.alloc(16 * n)
    L.chk(L.lib.hobbit_fill_splitmix(L.ctx, buf, n, 4242))
    out = {"lib": os.path.basename(args.lib), "forward_fft_batch_ms": {}, "launch_counts_forward": {}}
    for logn in range(13, 25):
        out["forward_fft_batch_ms"][str(logn)] = [round(L.time_ms("hobbit_fft_batch", buf, logn, 1, False, args.warmup, args.steps), 4) for _ in range(args.repeats)]
    for logn in COUNT_AT:
        out["launch_counts_forward"][str(logn)] = L.launch_counts("hobbit_fft_batch", buf, logn, False)
    if top == 28:
        out["inverse_fft_any_ms"] = {}; out["forward_fft_any_ms"] = {}; out["launch_counts_inverse"] = {}; out["callers"] = {}
        for logn in range(13, 29):
            out["inverse_fft_any_ms"][str(logn)] = [round(L.time_ms("hobbit_fft_any", buf, logn, 1, True, args.warmup, args.steps), 4) for _ in range(args.repeats)]
            if logn >= 25:
                out["forward_fft_any_ms"][str(logn)] = [round(L.time_ms("hobbit_fft_any", buf, logn, 1, False, args.warmup, args.steps), 4) for _ in range(args.repeats)]
        for logn in COUNT_AT + (25, 27):
            out["launch_counts_inverse"][str(logn)] = L.launch_counts("hobbit_fft_any", buf, logn, True)
        for logn, batch in ((17, 32), (23, 16)):
            for inv in (False, True):
                out["callers"]["2^%d x %d %s" % (logn, batch, "inverse" if inv else "forward")] = round(L.time_ms("hobbit_fft_any", buf, logn, batch, inv, args.warmup, args.steps), 4)
    L.lib.hobbit_free(L.ctx, buf)
    L.lib.hobbit_ctx_destroy(L.ctx)
    print("BENCH_FFT_WORKER " + json.dumps(out))


def run_worker(lib, args, forward_only):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    if forward_only:
        cmd.append("--forward-only")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("worker failed (%d) for %s" % (r.returncode, lib))
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_FFT_WORKER ")][-1]
    return json.loads(line[len("BENCH_FFT_WORKER "):])


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libhobbit_hip.so built from the parent commit")
    ap.add_argument("--lib", default=os.environ.get("HOBBIT_HIP_LIB") or os.path.join(PKG, "libhobbit_hip.so"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_any_length.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--forward-only", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    doc = {"what": "hobbit_fft_batch / hobbit_fft_any, HIP-event ms, median of %d after %d warm-up calls, %d repeats each" % (args.steps, args.warmup, args.repeats)}
    if args.parent:                                     # parent, this, parent: the parent's spread brackets this build's run
        p1 = run_worker(os.path.abspath(args.parent), args, True)
        this = run_worker(args.lib, args, False)
        p2 = run_worker(os.path.abspath(args.parent), args, True)
        doc["parent"] = {"forward_fft_batch_ms": {k: p1["forward_fft_batch_ms"][k] + p2["forward_fft_batch_ms"][k] for k in p1["forward_fft_batch_ms"]},
                         "launch_counts_forward": p1["launch_counts_forward"]}
    else:
        this = run_worker(args.lib, args, False)
    doc["this"] = this
    fwd = {int(k): med(v) for k, v in this["forward_fft_batch_ms"].items()}
    fwd.update({int(k): med(v) for k, v in this["forward_fft_any_ms"].items()})
    inv = {int(k): med(v) for k, v in this["inverse_fft_any_ms"].items()}
    doc["inverse_over_forward"] = {str(k): round(inv[k] / fwd[k], 3) for k in sorted(inv)}
    if args.parent:
        cmpd = {}
        for k, v in doc["parent"]["forward_fft_batch_ms"].items():
            t = med(this["forward_fft_batch_ms"][k])
            cmpd[k] = {"parent_min": min(v), "parent_max": max(v), "this_median": t, "this_min": min(this["forward_fft_batch_ms"][k]),
                       "inside_parent_spread": bool(min(v) <= t <= max(v)), "faster_than_parent_min": bool(t < min(v))}
        doc["forward_vs_parent"] = cmpd
        doc["launch_counts_identical"] = doc["parent"]["launch_counts_forward"] == this["launch_counts_forward"]
    per_el_24 = fwd[24] / ((1 << 24) * 24)
    doc["long"] = {}
    for k in (25, 26, 27, 28):
        for name, t in (("forward", fwd[k]), ("inverse", inv[k])):
            doc["long"]["2^%d %s" % (k, name)] = {"ms": round(t, 3), "sweeps": SWEEPS[k],
                                                  "fraction_of_hbm_peak": round(SWEEPS[k] * 32.0 * (1 << k) / (t * 1e-3) / (HBM_TBS * 1e12), 3),
                                                  "time_per_element_log_vs_2^24_forward": round(t / ((1 << k) * k) / per_el_24, 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": args.out, "forward_2^24_ms": fwd[24], "2^28_forward_ms": fwd[28], "2^28_inverse_ms": inv[28],
                      "launch_counts_identical": doc.get("launch_counts_identical")}))


if __name__ == "__main__":
    main()
