"""Turn two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE; separate runs, as MI355X_MICROARCH.md prescribes) of the same bench command
into HBM bytes per launch and kernel.  gfx950 corrections per the guide: counters are in KB; FETCH_SIZE reports half the bytes of
wide coalesced reads, so it is doubled.  usage: hbm_traffic.py <fetch counter_collection.csv> <write counter_collection.csv> <out.json> <command...>"""
import collections, csv, json, sys

def load(path, counter):
    acc = collections.defaultdict(lambda: [0.0, 0])
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] != counter:
            continue
        full = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("hobbit::", "")
        name = full.split("<")[0]
        if name == "k_enc_fat":                               # one template: C_0 has two outputs per lane, C_1 one, D_0 three
            name = "k_enc_fat_" + {"2": "A", "1": "C1", "3": "D"}.get(full.split("<")[1][:1], "?")
        elif name.startswith("k_encode"):                     # the one-workgroup-per-column passes are one template: tell them apart by their workgroup size
            wgs = int(r["Workgroup_Size"])                    # (of these, the in-place chain of trs = 4096, the 2^28 workload, launches only k_encode_M2)
            name = "k_encode_A" if wgs > 512 else "k_encode_M2" if wgs <= 128 else "k_encode_B"
        a = acc[name]; a[0] += float(r["Counter_Value"]); a[1] += 1
    return acc

fetch, write = load(sys.argv[1], "FETCH_SIZE"), load(sys.argv[2], "WRITE_SIZE")
out = {"command": " ".join(sys.argv[4:]), "note": "FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 reports half the bytes of wide coalesced reads); units KB->bytes", "kernels": {}}
for k in sorted(set(fetch) | set(write)):
    n = max(fetch[k][1], write[k][1], 1)
    f = 2.0 * 1024.0 * fetch[k][0] / n; w = 1024.0 * write[k][0] / n
    out["kernels"][k] = {"launches": n, "fetch_bytes_per_launch_corrected": f, "write_bytes_per_launch": w, "hbm_bytes_per_launch": f + w}
json.dump(out, open(sys.argv[3], "w"), indent=1)
for k, v in out["kernels"].items():
    if v["hbm_bytes_per_launch"] > 1e9:
        print("%-20s %8.3f GB per launch (%d launches)" % (k, v["hbm_bytes_per_launch"] / 1e9, v["launches"]))
