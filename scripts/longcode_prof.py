"""scripts/longcode_prof.py -- commit + open of Our_PC at tensor_row_size 8192 (test_PC(2^28, 4, 16)): wall times, the per-kernel split from
HIP events, and the long-code encode kernels against the HBM roof and the multiply-add floor.

The comparison point is the n = 4096 encode of test_PC(2^28, 4, 32): 6.65 ms for the same 2^28 message (BENCH_r03), 69 084 edges per column
on 32 x 4096 columns.

usage: python scripts/longcode_prof.py [--logn 28] [--K 16] [--steps 5] [--out gpu_out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
# multiply-add floor of the 96-bit accumulation: per edge and lane 4 v_mad_u64_u32 (half rate: 8 cycles per wave instruction on a SIMD) and
# 4 v_addc (full rate: 4 cycles) = 48 SIMD cycles per 64 edges; 1024 SIMDs at 2.4 GHz
MAD_FLOOR_EDGES_PER_S = 1024 * 2.4e9 * 64 / 48.0
REF_4096 = {"ms": 6.65, "edges_per_column": 69084, "columns": 32 * 4096}      # BENCH_r03: encode of test_PC(2^28, 4, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from __graft_entry__ import load_package
    hb = load_package().Hobbit(0)
    N, K = 1 << a.logn, a.K
    trs = N // (K << 11)
    cols = 2 * (N // K) // trs
    ncols = K * cols                                          # codewords encoded per commit
    hb.rng_reset()
    code_len = hb.expander_init_store(trs)
    lv = hb._graph_levels                                     # (dep, kind) -> (L, R, degree, nbr, w)
    edges = sum(int(L) * int(d) for (L, R, d, _, _) in lv.values())
    d = hb.fill_splitmix(N, 7)
    x = hb.generate_randomness(a.logn)

    def run(steps, do_open):
        t_c = t_o = 0.0
        for _ in range(steps):
            t0 = time.perf_counter()
            c = hb.commit_standard((d, N), K, trs, 1)
            t1 = time.perf_counter()
            if do_open:
                res = hb.open_standard((d, N), c, x, 5900, want_paths=False)
                assert res["checks"].tolist() == [1, 1, 1]
            t2 = time.perf_counter()
            c.free()
            t_c += t1 - t0; t_o += t2 - t1
        return 1e3 * t_c / steps, 1e3 * t_o / steps

    run(2, True)                                              # warm-up: allocations, graphs, twiddles
    commit_ms, open_ms = run(a.steps, True)
    hb.profile(True); hb.profile_reset()
    run(a.steps, False)                                       # commit alone under the per-kernel events
    prof = hb.profile_report()
    hb.profile(False)
    kern = {k: {"ms_per_commit": v[0] / a.steps, "launches_per_commit": v[1] / a.steps} for k, v in sorted(prof.items())}

    # bytes each encode kernel moves per commit (HBM: its input window in, its outputs out) and the edges it multiplies
    n = trs; deps = sorted({dep for dep, _ in lv}); D = len(deps)
    nd = [n] + [lv[(j, 0)][1] for j in deps]
    cw = [0] * (D + 1); cw[D] = nd[D]
    for j in reversed(deps):
        cw[j] = nd[j] + cw[j + 1] + lv[(j, 1)][1]
    depth = next(j for j in range(D + 1) if cw[j] <= 4096)    # TILE_MID_MAX: the sub-codeword left to the one-pass kernel
    split = {"k_enc_tiled_C": [0, 0], "k_enc_tiled_D": [0, 0], "k_encode_long_M": [0, 0]}
    for j in range(depth):
        L, R, dg = lv[(j, 0)][:3]; split["k_enc_tiled_C"][0] += 16 * (L + R); split["k_enc_tiled_C"][1] += L * dg
        L, R, dg = lv[(j, 1)][:3]; split["k_enc_tiled_D"][0] += 16 * (L + R); split["k_enc_tiled_D"][1] += L * dg
    split["k_enc_tiled_D"][0] += 16 * (((code_len + 3) & ~3) - code_len)
    split["k_encode_long_M"][0] = 16 * cw[depth] if depth <= D else 0
    split["k_encode_long_M"][1] = edges - split["k_enc_tiled_C"][1] - split["k_enc_tiled_D"][1]
    roof = {}
    enc_ms = 0.0
    for k, (b, e) in split.items():
        if k not in kern:
            continue
        ms = kern[k]["ms_per_commit"]; enc_ms += ms
        gb = b * ncols / 1e9; ge = e * ncols
        roof[k] = {"ms_per_commit": ms, "algorithmic_GB": gb, "achieved_GBs": gb / (ms * 1e-3), "frac_hbm": gb / (ms * 1e-3) / HBM_PEAK_GBS,
                   "edges": ge, "edges_per_s": ge / (ms * 1e-3), "frac_mad_floor": ge / (ms * 1e-3) / MAD_FLOOR_EDGES_PER_S}
    ref_edges = REF_4096["edges_per_column"] * REF_4096["columns"]
    ns_edge = enc_ms * 1e6 / (edges * ncols); ref_ns_edge = REF_4096["ms"] * 1e6 / ref_edges
    out = {"shape": {"logN": a.logn, "K": K, "trs": trs, "code_len": code_len, "columns": ncols, "edges_per_column": edges, "tiled_depth": depth},
           "commit_ms": commit_ms, "open_ms": open_ms, "kernels": kern, "roofline_kernels": roof,
           "encode": {"ms_per_commit": enc_ms, "ns_per_edge": ns_edge, "n4096_ns_per_edge": ref_ns_edge, "ratio_vs_n4096": ns_edge / ref_ns_edge,
                      "mad_floor_ms": edges * ncols / MAD_FLOOR_EDGES_PER_S * 1e3}}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s)
    d.free()
    hb.close()


if __name__ == "__main__":
    main()
