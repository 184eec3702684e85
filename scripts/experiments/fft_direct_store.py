"""Experiment (iv)(d), DESIGN.md section 4: the row FFT stores the codeword-major tensor itself, each column's message half rotated.

Needs the library built with fft_direct_store.patch applied (HOBBIT_EXP_DIRECT selects the variant per commit).  Commit-only loop at the
flagship shape (2^28, K = 32, trs = 4096); the variants alternate, ROUNDS rounds of REPS commits each after one warm-up commit.

    python scripts/experiments/fft_direct_store.py OUT.json [variant ...]

Per variant and round, ms per commit: phase_rows (first row-FFT start to last FFT / transpose end), k_fft4096, k_transpose, k_enc_fat_A.
With S != 0 the rest of the commit reads a layout it does not know: its timings stand, its root does not.
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from __graft_entry__ import load_package

out_path = sys.argv[1]
variants = sys.argv[2:] or ["off", "0", "128", "256", "512", "1024", "4096", "xor"]
ROUNDS, REPS = int(os.environ.get("ROUNDS", "4")), int(os.environ.get("REPS", "5"))
mod = load_package(); hb = mod.Hobbit(0)
N, K = 1 << 28, 32
trs = N // (K << 11)
hb.rng_reset(); hb.expander_init_store(trs)
p = hb.fill_splitmix(N, 5)
res = {v: [] for v in variants}
roots = {}
for rnd in range(ROUNDS):
    for v in variants:
        os.environ["HOBBIT_EXP_DIRECT"] = v
        c = hb.commit_standard((p, N), K, trs, 1); roots.setdefault(v, bytes(c.root()).hex()); c.free()      # warm-up in this variant
        hb.profile(True); hb.profile_reset()
        for _ in range(REPS):
            c = hb.commit_standard((p, N), K, trs, 1); c.free()
        hb.sync()
        rep = hb.profile_report(); hb.profile(False)
        row = {k: round(rep[k][0] / REPS, 4) for k in ("phase_rows", "k_fft4096", "k_transpose", "k_enc_fat_A", "k_leaf_chain") if k in rep}
        res[v].append(row)
        print(rnd, v, row, flush=True)
summary = {}
for v in variants:
    ph = [r["phase_rows"] for r in res[v]]
    summary[v] = {"phase_rows_mean": round(sum(ph) / len(ph), 4), "phase_rows_spread": round(max(ph) - min(ph), 4), "root": roots[v]}
json.dump({"shape": {"logn": 28, "K": K, "trs": trs}, "rounds": ROUNDS, "reps": REPS, "per_round_ms": res, "summary": summary}, open(out_path, "w"), indent=1)
print(json.dumps(summary))
hb.close()
