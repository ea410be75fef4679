#!/usr/bin/env python3
"""Cost of a view: the stand-in at 1920x1080 rendered through a generic look-at view against the same
render with the NULL view, alternated in one run, for a pinhole camera and for a thin lens (radius != 0).

    python tools/view_cost.py [--spp 16] [--rounds 5] [--integrator 0]

Prints one JSON line per camera: the median device time of the render (`seconds`), of the integration kernel
(`kernel_ms`) and of everything else -- the set-up kernel, where a pinhole unit's rotation runs, once per pixel --
as seconds - kernel_ms, for the NULL view and for the view.  The two renders are different images (the view looks
elsewhere), so this is the cost of the code path on a comparable shot, not of the same rays.
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
    a = ap.parse_args()
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    pos = (0.0, 1.0, 3.0)
    with pt.Renderer(s, 0) as r:
        for radius in (0.0, 0.05):
            cam = pt.make_camera(pos, 1.0, 3.0, radius, a.width, a.height)
            # a generic view: a few degrees off the reference pose, square pixels at the reference's vertical extent
            view = pt.look_at(pos, (0.3, 0.9, 0.0), (0.05, 1.0, 0.02))
            view.film_w = a.width / a.height
            shots = {"null": None, "view": view}
            t = {k: dict(seconds=[], kernel_ms=[]) for k in shots}
            for k, v in shots.items():                       # warm-up: tables, buffers
                r.render(cam, a.width, a.height, 1, 3, a.integrator, 1234, view=v)
            for _ in range(a.rounds):
                for k, v in shots.items():                   # alternated
                    _, st = r.render(cam, a.width, a.height, a.spp, 3, a.integrator, 1234, view=v)
                    t[k]["seconds"].append(st["seconds"])
                    t[k]["kernel_ms"].append(st["kernel_ms"])
            out = dict(radius=radius, integrator=a.integrator, width=a.width, height=a.height, spp=a.spp, rounds=a.rounds)
            for k in shots:
                sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
                out[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms,
                              seconds_min=min(t[k]["seconds"]), seconds_max=max(t[k]["seconds"]))
            print(json.dumps(out))


if __name__ == "__main__":
    main()
