#!/usr/bin/env python3
"""Cost of temporal reprojection: the stand-in at 1920x1080, per frame one 1-spp render, one feature pass
and one pt_temporal_push_device, for a still camera and for a pan of about 2 pixels per frame, alternated in one run.

    python tools/temporal_cost.py [--frames 12] [--rounds 5] [--shift 2.0] [--out FILE.json]

Prints one JSON line: per mode the median host wall time of each blocking call (every call ends in a device
synchronise) and the render's own device time (`seconds` of its stats), the median and the largest reprojection
distance in pixels measured on the last frame's features (pt.project through the previous camera), the share of the
pixels that kept a history, and the traffic floor of the push: (60 B own input + 56 B of history read once + 72 B
written) per pixel over 8 TB/s and over the 6.29 TB/s a float4 copy reaches.  The kernel's own time (`tp_push`) comes
from running this script under `rocprofv3 --kernel-trace --stats`, in a run of its own.  --out also keeps the line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cudapathtracer_amd as pt  # noqa: E402
from cudapathtracer_amd import scenes  # noqa: E402

OWN_B, TAP_B, WRITE_B = 60, 56, 72


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shift", type=float, default=2.0, help="pixels per frame at the image centre (the pan's angle)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = a.width, a.height
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)
    pos = scenes.SPONZA_STANDIN_CAMERA["pos"]
    step = a.shift / W          # a pan by this angle moves the centre of a unit film at distance 1 by `shift` pixels

    def view(mode, i):
        th = step * i if mode == "pan" else 0.0
        return pt.look_at(pos, (pos[0] + math.sin(th), pos[1], pos[2] - math.cos(th)))

    img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    out = torch.zeros_like(img)
    var = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    feat = torch.zeros(H * W * 48, dtype=torch.uint8, device="cuda")
    modes = ("still", "pan")
    wall = {m: dict(render=[], render_device_s=[], features=[], push=[]) for m in modes}
    res = {}
    with pt.Renderer(s, 0) as r, r.temporal(W, H) as t:
        for rnd in range(a.rounds + 1):                     # (round 0: warm-up)
            for m in modes:                                 # alternated
                t.reset()
                for i in range(a.frames):
                    v = view(m, i)
                    img.zero_()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    st = r.render_device(cam, img.data_ptr(), W, H, 1, seed=1234 + i, view=v)
                    t1 = time.perf_counter()
                    r.features_device(cam, feat.data_ptr(), W, H, view=v)
                    t2 = time.perf_counter()
                    t.push_device(img.data_ptr(), feat.data_ptr(), out.data_ptr(), cam, v, d_var_ptr=var.data_ptr())
                    t3 = time.perf_counter()
                    if rnd and i:                           # (frame 0 has no history to gather)
                        wall[m]["render"].append(t1 - t0)
                        wall[m]["render_device_s"].append(st["seconds"])
                        wall[m]["features"].append(t2 - t1)
                        wall[m]["push"].append(t3 - t2)
                if rnd == a.rounds:
                    n = t.history_length()
                    f = np.frombuffer(feat.cpu().numpy().tobytes(), dtype=pt.FEATURE).reshape(H, W)
                    prev = view(m, a.frames - 2)
                    d = []
                    for y in range(4, H, 97):
                        for x in range(4, W, 101):
                            if f["prim"][y, x] >= 0:
                                front, sx, sy = pt.project(cam, f["position"][y, x], prev)
                                if front:
                                    d.append(math.hypot(sx - x, sy - y))
                    hit = f["prim"] >= 0
                    res[m] = dict(move_px_median=statistics.median(d), move_px_max=max(d), sampled=len(d),
                                  hit_fraction=float(hit.mean()), kept_history_fraction=float((n[hit] > 1).mean()),
                                  history_length_max=float(n.max()), finite_variance_fraction=float(torch.isfinite(var).float().mean()))
    bytes_px = OWN_B + TAP_B + WRITE_B
    line = dict(width=W, height=H, frames=a.frames, rounds=a.rounds, shift=a.shift,
                push_bytes_per_pixel=bytes_px, push_bytes_per_pixel_uncached_taps=OWN_B + 4 * TAP_B + WRITE_B,
                floor_us_8TBs=W * H * bytes_px / 8e12 * 1e6, floor_us_copy_6p29TBs=W * H * bytes_px / 6.29e12 * 1e6)
    for m in modes:
        line[m] = dict({k + "_ms_median": statistics.median(v) * 1e3 for k, v in wall[m].items()},
                       push_ms_min=min(wall[m]["push"]) * 1e3, push_ms_max=max(wall[m]["push"]) * 1e3, **res[m])
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
