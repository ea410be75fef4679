#!/usr/bin/env python3
"""Per-kernel device times of tools/gpu/denoise_cost.py from its rocprofv3 kernel trace.

usage: denoise_cost_report.py <run_kernel_trace.csv> [W H]
The denoiser's dispatches come in calls of 7 (dn_prepass, 5 x dn_iterate, dn_finish); a call is "tiled" when its
first iteration is dn_iterate<true>, else "direct"; the first call of each kind is the warm-up and is dropped.
Prints one JSON object: per kernel the times of every repeat (us), their median, each iteration's ratio to the
direct gather's and to its traffic floor -- (bytes read once + bytes written once) / 8 TB/s, 64 B per pixel
per iteration (48 B of planes in, 16 B out), 76 + 64 B for the prepass, 44 + 12 B for the last pass."""
import csv
import json
import statistics
import sys

path = sys.argv[1]
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) >= 4 else (1920, 1080)
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
staged_name = lambda n: "dn_iterate<true>" in n or "dn_iterateILb1" in n
us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
feat = [us(r) for r in rows if "primary_features" in r["Kernel_Name"]][1:]
dn = [r for r in rows if "dn_" in r["Kernel_Name"]]
assert len(dn) % 7 == 0, len(dn)
calls = {"tiled": [], "direct": []}
for k in range(0, len(dn), 7):
    c = dn[k:k + 7]
    names = [r["Kernel_Name"] for r in c]
    assert "dn_prepass" in names[0] and "dn_finish" in names[6] and all("dn_iterate" in n for n in names[1:6]), names
    calls["tiled" if staged_name(names[1]) else "direct"].append(c)
PEAK = 8e12
px = W * H
floor_us = {"prepass": px * (76 + 64) / PEAK * 1e6, "finish": px * (44 + 12) / PEAK * 1e6}
labels = ["prepass"] + ["iterate_step_%d" % (1 << i) for i in range(5)] + ["finish"]
for l in labels[1:6]:
    floor_us[l] = px * 64 / PEAK * 1e6
out = {"image": [W, H], "traffic_floor_us": {k: round(v, 2) for k, v in floor_us.items()},
       "primary_features_us": [round(x, 1) for x in feat], "kernels": {}}
med = {}
for mode, cs in calls.items():
    cs = cs[1:]   # (warm-up)
    for i, l in enumerate(labels):
        t = [us(c[i]) for c in cs]
        staged = [staged_name(c[i]["Kernel_Name"]) for c in cs]
        med[(mode, l)] = statistics.median(t)
        out["kernels"].setdefault(l, {})[mode] = {"us": [round(x, 1) for x in t], "median_us": round(med[(mode, l)], 1),
                                                  "lds_staged": bool(staged and staged[0])}
    out["kernels"].setdefault("total", {})[mode] = {"us": [round(sum(us(r) for r in c), 1) for c in cs]}
for l in labels:
    k = out["kernels"][l]
    k["tiled_over_direct"] = round(med[("tiled", l)] / med[("direct", l)], 3)
    k["tiled_over_floor"] = round(med[("tiled", l)] / floor_us[l], 2)
    k["direct_over_floor"] = round(med[("direct", l)] / floor_us[l], 2)
print(json.dumps(out, indent=1))
