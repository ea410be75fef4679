#!/usr/bin/env python3
"""What the variance-guided filter costs on C3's frame (stand-in, 1920x1080), against the plain filter in the same
process: an accumulator of 4 passes of 1 sample with a noise estimator gives the image and the variance map; then,
REPS times after one warm-up round, the calls of MODES in turn -- pt_noise_variance_device, pt_denoise_device with
default parameters (the yardstick), and pt_denoise_guided_device with default parameters on the default kernels, with
every step staged through LDS (PT_DENOISE_TILED_MAX=16) and on the direct gather (PT_DENOISE_DIRECT=1).  The three
guided outputs must be equal in every byte.  Meant to run under `rocprofv3 --kernel-trace`
(tools/gpu/denoise_guided_cost.sh); tools/gpu/denoise_guided_cost_report.py turns the trace into per-kernel times.
Prints one JSON line (host wall times)."""
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

W, H, PASSES, BOUNCES = 1920, 1080, 4, 3
REPS = int(os.environ.get("REPS", "3"))
MODES = ("variance", "plain", "guided", "guided_staged", "guided_direct")   # the report relies on this order


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
    var = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    out = {m: torch.zeros_like(img) for m in MODES[1:]}
    wall = {m: [] for m in MODES}
    with pt.Renderer(s, 0) as r:
        r.features_device(cam, feat.data_ptr(), W, H)
        with r.accumulator(cam, W, H, bounces=BOUNCES) as acc, acc.noise() as est:
            for _ in range(PASSES):
                acc.add(1, d_out_ptr=img.data_ptr())
                est.update()
            for rep in range(REPS + 1):   # (rep 0: warm-up)
                for mode in MODES:
                    os.environ.pop("PT_DENOISE_DIRECT", None)
                    os.environ.pop("PT_DENOISE_TILED_MAX", None)
                    if mode == "guided_staged":
                        os.environ["PT_DENOISE_TILED_MAX"] = "16"
                    if mode == "guided_direct":
                        os.environ["PT_DENOISE_DIRECT"] = "1"
                    t = time.perf_counter()
                    if mode == "variance":
                        est.variance_device(var.data_ptr())
                    elif mode == "plain":
                        r.denoise_device(img.data_ptr(), feat.data_ptr(), out[mode].data_ptr(), W, H)
                    else:
                        r.denoise_guided_device(img.data_ptr(), feat.data_ptr(), var.data_ptr(), out[mode].data_ptr(), W, H)
                    wall[mode].append(time.perf_counter() - t)
        torch.cuda.synchronize()
        same = bool(torch.equal(out["guided"], out["guided_staged"]) and torch.equal(out["guided"], out["guided_direct"]))
        differs = not bool(torch.equal(out["guided"], out["plain"]))
        known = float(torch.isfinite(var).float().mean())
    print(json.dumps({"config": [W, H, PASSES, BOUNCES], "reps": REPS, "modes": MODES, "wall_s_first_is_warmup": wall,
                      "guided_kernels_agree": same, "guided_differs_from_plain": differs,
                      "finite_variance_fraction": round(known, 4)}))
    if not same or not differs:
        sys.exit("denoise_guided_cost: the guided kernels disagree, or the variance changed nothing")


if __name__ == "__main__":
    main()
