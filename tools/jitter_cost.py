#!/usr/bin/env python3
"""Cost of sub-pixel jitter: the stand-in at 1920x1080 rendered with PT_FLAG_JITTER (box and tent)
against the same render without it, alternated in one run, for a pinhole camera and for a thin lens (radius != 0).

    python tools/jitter_cost.py [--spp 16] [--rounds 5] [--integrator 0] [--out FILE.json]

Prints one JSON line per camera: the median device time of the render (`seconds`), of the integration kernel
(`kernel_ms`) and of everything else -- the set-up kernel -- as seconds - kernel_ms, for the plain render and the two
jittered ones, with the traced-ray counts; and one last line of ratios: jittered pinhole / plain pinhole (the price of
losing the primary-hit memo: one more traced ray per sample), jittered pinhole / plain lens (that render also forms
and traces a camera ray per sample, with more arithmetic per ray), jittered lens / plain lens.  --out also keeps the
lines in a file.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudapathtracer_amd as pt  # noqa: E402
from cudapathtracer_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--integrator", type=int, default=0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    kinds = {"plain": 0, "box": pt.PT_FLAG_JITTER, "tent": pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT}
    lines, med = [], {}
    with pt.Renderer(s, 0) as r:
        for radius in (0.0, 0.05):
            cam = pt.make_camera((0.0, 1.0, 3.0), 1.0, 3.0, radius, a.width, a.height)
            t = {k: dict(seconds=[], kernel_ms=[]) for k in kinds}
            rays = {}
            for k, f in kinds.items():                       # warm-up: tables, buffers
                r.render(cam, a.width, a.height, 1, 3, a.integrator, 1234, f)
            for _ in range(a.rounds):
                for k, f in kinds.items():                   # alternated
                    _, st = r.render(cam, a.width, a.height, a.spp, 3, a.integrator, 1234, f)
                    t[k]["seconds"].append(st["seconds"])
                    t[k]["kernel_ms"].append(st["kernel_ms"])
                    rays[k] = dict(rays_traced=st["rays_traced"], rays_reference=st["rays_reference"], split_pixels=st["split_pixels"])
            out = dict(radius=radius, integrator=a.integrator, width=a.width, height=a.height, spp=a.spp, rounds=a.rounds)
            for k in kinds:
                sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
                out[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms, seconds_min=min(t[k]["seconds"]),
                              seconds_max=max(t[k]["seconds"]), **rays[k])
                med[(radius, k)] = sec
            lines.append(out)
    lines.append(dict(ratios=dict(
        box_pinhole_over_plain_pinhole=med[(0.0, "box")] / med[(0.0, "plain")],
        tent_pinhole_over_plain_pinhole=med[(0.0, "tent")] / med[(0.0, "plain")],
        box_pinhole_over_plain_lens=med[(0.0, "box")] / med[(0.05, "plain")],
        box_lens_over_plain_lens=med[(0.05, "box")] / med[(0.05, "plain")],
        tent_lens_over_plain_lens=med[(0.05, "tent")] / med[(0.05, "plain")])))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
