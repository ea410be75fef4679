#!/usr/bin/env python3
"""What a denoised preview costs on C3's frame (stand-in, 1920x1080): primary_features, then pt_denoise_device
with default parameters (5 iterations), REPS times alternating the LDS-staged kernel for every step
(PT_DENOISE_TILED_MAX=16) with the direct gather (PT_DENOISE_DIRECT=1), after one warm-up call of each.  The two
outputs must be equal in every byte.  Meant to run under `rocprofv3 --kernel-trace` (tools/gpu/denoise_cost.sh);
tools/gpu/denoise_cost_report.py turns the trace into per-kernel times.  Prints one JSON line (host wall times)."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cudapathtracer_amd as pt  # noqa: E402
from cudapathtracer_amd import scenes  # noqa: E402

W, H, SPP, BOUNCES = 1920, 1080, 4, 3
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
    img = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    feat = torch.zeros(H * W * 48, dtype=torch.uint8, device="cuda")
    out = {"tiled": torch.zeros_like(img), "direct": torch.zeros_like(img)}
    wall = {"tiled": [], "direct": [], "features": []}
    with pt.Renderer(s, 0) as r:
        r.render_device(cam, img.data_ptr(), W, H, SPP, bounces=BOUNCES)
        for rep in range(REPS + 1):   # (rep 0: warm-up)
            t = time.perf_counter()
            r.features_device(cam, feat.data_ptr(), W, H)
            wall["features"].append(time.perf_counter() - t)
            for mode in ("tiled", "direct"):
                os.environ.pop("PT_DENOISE_DIRECT", None)
                os.environ["PT_DENOISE_TILED_MAX"] = "16"
                if mode == "direct":
                    os.environ["PT_DENOISE_DIRECT"] = "1"
                t = time.perf_counter()
                r.denoise_device(img.data_ptr(), feat.data_ptr(), out[mode].data_ptr(), W, H)
                wall[mode].append(time.perf_counter() - t)
        torch.cuda.synchronize()
        same = bool(torch.equal(out["tiled"], out["direct"]))
        changed = not bool(torch.equal(out["tiled"], img))
    print(json.dumps({"config": [W, H, SPP, BOUNCES], "reps": REPS, "wall_s_first_is_warmup": wall,
                      "tiled_equals_direct": same, "filter_changed_the_image": changed}))
    if not same or not changed:
        sys.exit("denoise_cost: tiled and direct outputs differ, or the filter did nothing")


if __name__ == "__main__":
    main()
