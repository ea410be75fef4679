#!/usr/bin/env python3
"""What the noise estimator costs on C3's frame (stand-in, 1920x1080, 3 bounces).

  noise_cost.py                       the workload: an accumulator with an estimator attached; after a warm-up round,
                                      REPS rounds of {1-spp pass, update (fold + summary), error map to a device
                                      buffer, update again (summary only)}.  Prints one JSON line: the pass's device
                                      time (pt_stats.seconds) and the host wall time of each step.  Meant to run under
                                      `rocprofv3 --kernel-trace --stats` (tools/gpu/noise_cost.sh), no counters.
  noise_cost.py --report TRACE.csv RUN.json
                                      per-kernel device times from that trace (the warm-up round dropped): every
                                      repeat, the median, the ratio to the traffic floor -- (bytes read once + bytes
                                      written once) / 8 TB/s -- and to the 1-spp pass measured in the same run.
Bytes per work slot: noise_update<true> reads mean 24 + prev 24 + mu, m2 16 + index 4 and writes prev 24 + mu, m2 16
(108 B); noise_update<false> reads mu, m2 16 + index 4 (20 B); noise_map reads the same and writes 4 (24 B)."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W, H, BOUNCES = 1920, 1080, 3
REPS = int(os.environ.get("REPS", "3"))
PEAK = 8e12
BYTES = {"noise_update<true>": 108, "noise_update<false>": 20, "noise_map": 24}


def run():
    import ctypes as C

    import torch

    import cudapathtracer_amd as pt
    from cudapathtracer_amd import _lib, scenes
    d = os.path.join(tempfile.gettempdir(), "pt_bench_scene")
    p = os.path.join(d, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(d)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)
    emap = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    wall = {"pass": [], "update_fold": [], "map": [], "update_summary": []}
    pass_dev, summaries = [], []
    npar = _lib.NoiseParams(0.05, 0.01)

    def timed(key, fn):
        t = time.perf_counter()
        r = fn()
        wall[key].append(time.perf_counter() - t)
        return r

    with pt.Renderer(s, 0) as r:
        r.render(cam, W, H, 2, bounces=BOUNCES)   # warm-up: jump tables, buffers
        with r.accumulator(cam, W, H, bounces=BOUNCES) as acc, acc.noise() as est:
            for rep in range(REPS + 1):   # (rep 0: warm-up)
                st = timed("pass", lambda: acc.add(1))
                pass_dev.append(st["seconds"])
                summaries.append(timed("update_fold", lambda: est.update()))
                timed("map", lambda: _lib.check(_lib.lib().pt_noise_map_device(est._h, C.byref(npar), C.c_void_p(emap.data_ptr()), None)))
                again = timed("update_summary", lambda: est.update())
                if again != summaries[-1]:
                    sys.exit("noise_cost: the summary-only update disagrees with the folding one")
            finite = int(torch.isfinite(emap).sum().item())
    last = summaries[-1]
    print(json.dumps({"config": [W, H, BOUNCES], "reps": REPS, "pass_device_s_first_is_warmup": pass_dev,
                      "wall_s_first_is_warmup": wall, "batches": last["batches"], "pixels": last["pixels"],
                      "converged": last["converged"], "finite_map_values": finite}))
    if last["batches"] != REPS + 1 or last["pixels"] != W * H or finite != W * H:
        sys.exit("noise_cost: unexpected summary")


def report(trace, run_json):
    import csv
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    def kind(name):
        if "noise_map" in name:
            return "noise_map"
        if "noise_update" in name:
            return "noise_update<true>" if ("<true>" in name or "ILb1" in name) else "noise_update<false>"
        return None

    times = {k: [] for k in BYTES}
    for r in rows:
        k = kind(r["Kernel_Name"])
        if k:
            times[k].append(us(r))
    info = json.loads(open(run_json).read().strip().splitlines()[-1])
    slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
    pass_us = [x * 1e6 for x in info["pass_device_s_first_is_warmup"][1:]]
    pass_med = statistics.median(pass_us)
    out = {"image": [W, H], "slots": slots, "pass_1spp_device_us": [round(x, 1) for x in pass_us],
           "pass_1spp_median_us": round(pass_med, 1), "kernels": {}}
    for k, t in times.items():
        t = t[1:]   # (warm-up)
        assert len(t) == info["reps"], (k, len(t))
        floor = slots * BYTES[k] / PEAK * 1e6
        med = statistics.median(t)
        out["kernels"][k] = {"us": [round(x, 1) for x in t], "median_us": round(med, 1), "bytes_per_slot": BYTES[k],
                             "traffic_floor_us": round(floor, 2), "over_floor": round(med / floor, 2),
                             "share_of_1spp_pass": round(med / pass_med, 4)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3])
    else:
        run()
