#!/usr/bin/env python3
"""Per-kernel device times of tools/gpu/denoise_guided_cost.py from its rocprofv3 kernel trace.

usage: denoise_guided_cost_report.py <run_kernel_trace.csv> [W H]
The script's rounds are MODES in turn: one noise_variance dispatch, a plain call of 7 dispatches (dn_prepass,
5 x dn_iterate, dn_finish) and three guided calls of 12 (dg_prepass, 5 x (dg_blur, dg_iterate), dn_finish); the first
round is the warm-up and is dropped.  Prints one JSON object: per call kind and kernel the times of every repeat (us)
and their median, the totals, the guided-over-plain ratios, the staged-over-direct ratio of every guided step, and the
variance map against its traffic floor -- 16 B per pixel (4 B slot index, 8 B m2, 4 B out) at 8 TB/s."""
import csv
import json
import statistics
import sys

path = sys.argv[1]
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) >= 4 else (1920, 1080)
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
rows = [r for r in rows if any(k in r["Kernel_Name"] for k in ("dn_prepass", "dn_iterate", "dn_finish", "dg_", "noise_variance"))]
PLAIN = ["prepass"] + ["iterate_step_%d" % (1 << i) for i in range(5)] + ["finish"]
GUIDED = ["prepass"] + [n % (1 << i) for i in range(5) for n in ("blur_step_%d", "iterate_step_%d")] + ["finish"]
SHAPE = [("variance", ["variance"]), ("plain", PLAIN), ("guided", GUIDED), ("guided_staged", GUIDED), ("guided_direct", GUIDED)]
per_round = sum(len(l) for _, l in SHAPE)
assert len(rows) % per_round == 0 and len(rows) > per_round, (len(rows), per_round)
times = {m: {l: [] for l in labels} for m, labels in SHAPE}
staged = {}
k = per_round   # (skip the warm-up round)
while k < len(rows):
    for mode, labels in SHAPE:
        for l in labels:
            name = rows[k]["Kernel_Name"]
            want = {"variance": "noise_variance", "prepass": "dn_prepass" if mode == "plain" else "dg_prepass", "finish": "dn_finish"}.get(
                l, "dg_blur" if l.startswith("blur") else ("dn_iterate" if mode == "plain" else "dg_iterate"))
            assert want in name, (mode, l, name)
            times[mode][l].append(us(rows[k]))
            if l.startswith("iterate"):
                staged[(mode, l)] = "<true>" in name or "ILb1" in name
            k += 1
px = W * H
out = {"image": [W, H], "calls": {}}
tot = {}
for mode, labels in SHAPE:
    c = {l: {"us": [round(x, 1) for x in times[mode][l]], "median_us": round(statistics.median(times[mode][l]), 1)} for l in labels}
    for l in labels:
        if (mode, l) in staged:
            c[l]["lds_staged"] = staged[(mode, l)]
    reps = [sum(times[mode][l][i] for l in labels) for i in range(len(times[mode][labels[0]]))]
    tot[mode] = statistics.median(reps)
    c["total"] = {"us": [round(x, 1) for x in reps], "median_us": round(tot[mode], 1)}
    out["calls"][mode] = c
out["guided_over_plain"] = {m: round(tot[m] / tot["plain"], 3) for m in ("guided", "guided_staged", "guided_direct")}
out["staged_over_direct_by_step"] = {
    l: round(statistics.median(times["guided_staged"][l]) / statistics.median(times["guided_direct"][l]), 3)
    for l in GUIDED if l.startswith("iterate")}
floor = px * 16 / 8e12 * 1e6
out["variance_map"] = {"traffic_floor_us": round(floor, 2), "over_floor": round(tot["variance"] / floor, 2)}
print(json.dumps(out, indent=1))
