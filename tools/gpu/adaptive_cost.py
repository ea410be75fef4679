#!/usr/bin/env python3
"""What an adaptive pass costs on C3's scene (stand-in, 1920x1080, 3 bounces).

  adaptive_cost.py                    the workload: one plain accumulator and one per mask (seeded random masks that
                                      leave about 100%, 50%, 10% and 1% of the pixels active, and one clustered mask: a
                                      centred rectangle of 10% of the image active), each frozen after a first 4-spp
                                      pass; a warm-up 4-spp pass of each (the frozen ones build their active list in
                                      it), then REPS rounds of {uniform 4-spp pass, 4-spp pass of every mask},
                                      alternated.  Then, on the 50% accumulator, an estimator and REPS device freeze
                                      sweeps.  Prints one JSON line with every pass's device time (pt_stats.seconds:
                                      unit set-up + integration kernel) and kernel_ms.  Meant to run under
                                      `rocprofv3 --kernel-trace --stats` (tools/gpu/adaptive_cost.sh), no counters.
  adaptive_cost.py --report TRACE.csv RUN.json
                                      the medians; each active pass against  fraction x (uniform - FIXED) + FIXED  with
                                      FIXED = 1.0 ms (what a pass costs besides its samples); and the
                                      sweeps' kernel times from the trace against their traffic floor, (bytes read once +
                                      written once) / 8 TB/s.
Bytes: the compaction reads the 4-B frozen_at plane twice (count, scatter) and writes 4 B per active slot (the block
totals are 1/256 of that); noise_freeze reads index 4 + frozen_at 4 + mu, m2 16 + W_q, b_q 8 = 32 B per slot and writes
4 B per newly frozen slot; init_active_states reads 4 B of list + 24 B of XORWOW state and writes 52 B per active slot."""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W, H, BOUNCES, SPP = 1920, 1080, 3, 4
REPS = int(os.environ.get("REPS", "3"))
PEAK = 8e12
FIXED_MS = 1.0
MASKS = [("random_100", 1.0), ("random_50", 0.5), ("random_10", 0.1), ("random_1", 0.01), ("clustered_10", 0.1)]


def masks():
    """name -> frozen mask (H, W); the random ones freeze a seeded pseudo-random 1 - fraction of the pixels (at least
    one, so that the 100% case runs the active-list path too)."""
    import numpy as np
    rng = np.random.default_rng(20241019)
    out = {}
    for name, frac in MASKS:
        if name.startswith("random"):
            m = rng.random((H, W)) >= frac
            m[0, 0] = True
        else:
            m = np.ones((H, W), dtype=bool)
            hh, ww = int(H * frac ** 0.5), int(W * frac ** 0.5)
            m[(H - hh) // 2:(H - hh) // 2 + hh, (W - ww) // 2:(W - ww) // 2 + ww] = False
        out[name] = m
    return out


def run():
    import cudapathtracer_amd as pt
    from cudapathtracer_amd import scenes
    d = os.path.join(tempfile.gettempdir(), "pt_bench_scene")
    p = os.path.join(d, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(d)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)
    ms = masks()
    out = {"config": [W, H, BOUNCES, SPP], "reps": REPS, "active": {}, "uniform": [], "passes": {k: [] for k in ms},
           "first_pass_after_freeze": {}, "freeze": []}
    with pt.Renderer(s, 0) as r:
        r.render(cam, W, H, 2, bounces=BOUNCES)   # warm-up: jump tables, buffers
        uni = r.accumulator(cam, W, H, bounces=BOUNCES)
        accs = {k: r.accumulator(cam, W, H, bounces=BOUNCES) for k in ms}
        for a in [uni] + list(accs.values()):
            a.add(SPP)
        uni.add(SPP)
        for k, a in accs.items():
            a.freeze(ms[k])
            st = a.add(SPP)                       # (builds the active list)
            out["active"][k] = st["samples"] // SPP
            out["first_pass_after_freeze"][k] = {"seconds": st["seconds"], "kernel_ms": st["kernel_ms"]}
        for _ in range(REPS):
            st = uni.add(SPP)
            if st["samples"] != W * H * SPP:
                sys.exit("adaptive_cost: the uniform pass sampled %d" % st["samples"])
            out["uniform"].append({"seconds": st["seconds"], "kernel_ms": st["kernel_ms"]})
            for k, a in accs.items():
                st = a.add(SPP)
                if st["samples"] != out["active"][k] * SPP or st["split_pixels"] != 0:
                    sys.exit("adaptive_cost: %s sampled %d" % (k, st["samples"]))
                out["passes"][k].append({"seconds": st["seconds"], "kernel_ms": st["kernel_ms"]})
        # the freeze sweep: REPS sweeps on the 50% accumulator (tolerances rising, so that each freezes something)
        a = accs["random_50"]
        with a.noise() as est:
            for _ in range(2):
                a.add(SPP)
                est.update()
            for tol in [0.05 * 2 ** i for i in range(REPS + 1)]:   # (the first: warm-up)
                newly, active = est.freeze(tol=tol)
                out["freeze"].append({"tol": tol, "newly": newly, "active": active})
                a.add(1)                          # (rebuilds the list: one more compaction in the trace)
        for a in [uni] + list(accs.values()):
            a.close()
    print(json.dumps(out))


def report(trace, run_json):
    import csv
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
    info = json.loads(open(run_json).read().strip().splitlines()[-1])
    slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
    med = lambda v: statistics.median(v)          # noqa: E731
    uni_ms = [x["seconds"] * 1e3 for x in info["uniform"]]
    out = {"image": [W, H], "slots": slots, "spp": SPP, "fixed_ms": FIXED_MS,
           "uniform_pass_ms": [round(x, 3) for x in uni_ms], "uniform_pass_median_ms": round(med(uni_ms), 3), "masks": {}}
    for k, _ in MASKS:
        t = [x["seconds"] * 1e3 for x in info["passes"][k]]
        km = [x["kernel_ms"] for x in info["passes"][k]]
        frac = info["active"][k] / (W * H)
        model = frac * (med(uni_ms) - FIXED_MS) + FIXED_MS
        out["masks"][k] = {"active": info["active"][k], "fraction": round(frac, 5), "pass_ms": [round(x, 3) for x in t],
                           "median_ms": round(med(t), 3), "integration_kernel_median_ms": round(med(km), 3),
                           "model_ms": round(model, 3), "over_model": round(med(t) / model, 3),
                           "of_uniform": round(med(t) / med(uni_ms), 4)}
    times = {}
    for r in rows:
        for key in ("active_count", "active_scan", "active_scatter", "noise_freeze", "init_active_states", "noise_fill_pix"):
            if key in r["Kernel_Name"]:
                times.setdefault(key, []).append(round(us(r), 1))
    n = len(times.get("active_count", []))
    out["compaction"] = {"launches": n, "count_us": times.get("active_count"), "scan_us": times.get("active_scan"),
                         "scatter_us": times.get("active_scatter"),
                         "note": "in trace order: one per mask (random 100 / 50 / 10 / 1%, clustered 10%), then one "
                                 "after each freeze sweep"}
    if n:
        tot = [a + b + c for a, b, c in zip(times["active_count"], times["active_scan"], times["active_scatter"])]
        act = [info["active"][k] for k, _ in MASKS]
        floors = [(slots * 8 + a * 4) / PEAK * 1e6 for a in act]
        out["compaction"]["total_us"] = [round(x, 1) for x in tot]
        out["compaction"]["traffic_floor_us_per_mask"] = [round(x, 2) for x in floors]
        out["compaction"]["over_floor_per_mask"] = [round(t / f, 1) for t, f in zip(tot, floors)]
    fz = times.get("noise_freeze", [])[1:]        # (warm-up)
    if fz:
        floor = slots * 32 / PEAK * 1e6
        out["noise_freeze"] = {"us": fz, "median_us": round(med(fz), 1), "bytes_per_slot": 32,
                               "traffic_floor_us": round(floor, 2), "over_floor": round(med(fz) / floor, 2),
                               "sweeps": info["freeze"][1:]}
    out["init_active_states_us"] = times.get("init_active_states")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3])
    else:
        run()
