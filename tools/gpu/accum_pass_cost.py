#!/usr/bin/env python3
"""What accumulation costs on C3 (stand-in, 1920x1080, 256 spp, 3 bounces): the plain render against an
accumulator fed the same 256 samples as 1 x 256, 8 x 32 and 32 x 8 passes (Renderer.accumulator), each
repeated REPS times.  Rates are device time (pt_stats.seconds summed over the passes of a frame) and wall
time around the add() calls; the last frame's bytes must equal the plain render's.  Prints one JSON object.
Run through tools/gpu/accum_pass_cost.sh (time limit, stops at the first failure)."""
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import cudapathtracer_amd as pt  # noqa: E402
from cudapathtracer_amd import scenes  # noqa: E402

W, H, SPP, BOUNCES = 1920, 1080, 256, 3
REPS = int(os.environ.get("REPS", "3"))


def main():
    d = os.path.join(tempfile.gettempdir(), "pt_bench_scene")
    p = os.path.join(d, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(d)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)
    out = {"config": [W, H, SPP, BOUNCES], "reps": REPS, "rows": []}
    with pt.Renderer(s, 0) as r:
        r.render(cam, W, H, 8, bounces=BOUNCES)   # warm-up: jump tables, buffers
        dev, wall, img = [], [], None
        for _ in range(REPS):
            t = time.perf_counter()
            img, st = r.render(cam, W, H, SPP, bounces=BOUNCES)
            wall.append(time.perf_counter() - t)
            dev.append(st["seconds"])
        digest = hashlib.sha256(img.tobytes()).hexdigest()
        n = W * H * SPP
        out["rows"].append(dict(mode="plain render", passes=1, device_s=dev, wall_s_incl_copy=wall,
                                msamples_per_s_device=[n / x / 1e6 for x in dev], rays_traced=st["rays_traced"]))
        for passes, per in ((1, 256), (8, 32), (32, 8)):
            dev, wall, traced = [], [], 0
            for _ in range(REPS):
                with r.accumulator(cam, W, H, bounces=BOUNCES) as acc:
                    t = time.perf_counter()
                    sts = [acc.add(per) for _ in range(passes)]
                    wall.append(time.perf_counter() - t)
                    dev.append(sum(x["seconds"] for x in sts))
                    traced = sum(x["rays_traced"] for x in sts)
                    same = hashlib.sha256(acc.image().tobytes()).hexdigest() == digest
                if not same:
                    print(json.dumps(out))
                    sys.exit("accumulated frame (%d x %d) differs from the plain render" % (passes, per))
            out["rows"].append(dict(mode="accumulator %d x %d" % (passes, per), passes=passes, device_s=dev, wall_s=wall,
                                    msamples_per_s_device=[n / x / 1e6 for x in dev],
                                    msamples_per_s_wall=[n / x / 1e6 for x in wall], rays_traced=traced,
                                    digest_equals_plain=True))
    out["image_sha256"] = digest
    print(json.dumps(out))


if __name__ == "__main__":
    main()
