#!/usr/bin/env python3
"""Cost of lightmap finishing: the gutter fill of a 2048 x 2048 lightmap with about 30 % uncovered texels
in chart-like blobs at radius 4 and 16, against a device copy of the same bytes; and the lightmapped view of the
stand-in at 1920 x 1080, against the feature pass it reads and a copy of the same bytes.  All alternated in one run.

    python tools/lightmap_cost.py [--rounds 7] [--reps 10] [--out FILE.json]

Prints one JSON line: per operation the median over the rounds of the median host wall time of `reps` blocking calls
(every call ends in a device synchronise; the copies are timed the same way, torch's copy_ and a synchronise, so the
launch and synchronise overhead is in every figure alike), the bytes each moves at the least, and the ratios.  The
kernels' own times (`lm_dilate`, `lm_shade`) come from running this script under `rocprofv3 --kernel-trace --stats`, in
a run of its own.  --out also keeps the line.
"""
import argparse
import json
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


def chart_mask(M, cell, seed):
    """An M x M mask of rectangular charts, one per cell x cell block, each inset by 4..18 texels a side: about 30 %
    of the texels lie in the gutters between them."""
    rng = np.random.RandomState(seed)
    m = np.zeros((M, M), np.uint8)
    for cy in range(0, M, cell):
        for cx in range(0, M, cell):
            l, r, t, b = rng.randint(4, 19, size=4)
            m[cy + t:cy + cell - b, cx + l:cx + cell - r] = 1
    return m


def timed(fn, reps):
    w = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        w.append(time.perf_counter() - t0)
    return statistics.median(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--map", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M, W, H = a.map, a.width, a.height
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    nt = int(s.view().num_tris)
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)

    rng = np.random.RandomState(1)
    mask = chart_mask(M, 128, 2)
    lm = torch.from_numpy(rng.rand(M, M, 3).astype(np.float32)).cuda()
    lm_out = torch.zeros_like(lm)
    d_mask = torch.from_numpy(mask).cuda()
    # every triangle charted onto a small triangle of its own somewhere in the map, as an atlas would
    ua = rng.rand(nt, 2).astype(np.float32) * 0.98
    table = np.concatenate([ua, ua + np.float32([0.01, 0.0]), ua + np.float32([0.0, 0.01])], axis=1).astype(np.float32)
    d_table = torch.from_numpy(table).cuda()
    n = W * H
    d_feat = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    d_view = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    copy_a = torch.zeros(n * 30 // 4, dtype=torch.float32, device="cuda")     # 60 B per pixel read + written, as the view
    copy_b = torch.zeros_like(copy_a)

    with pt.Renderer(s, 0) as r:
        r.features_device(cam, d_feat.data_ptr(), W, H)
        ops = {
            "dilate_r4": lambda: r.lightmap_dilate_device(lm.data_ptr(), d_mask.data_ptr(), lm_out.data_ptr(), M, M, 4),
            "dilate_r16": lambda: r.lightmap_dilate_device(lm.data_ptr(), d_mask.data_ptr(), lm_out.data_ptr(), M, M, 16),
            "dilate_copy": lambda: lm_out.copy_(lm),
            "features": lambda: r.features_device(cam, d_feat.data_ptr(), W, H),
            "shade": lambda: r.lightmap_shade_device(d_feat.data_ptr(), n, d_table.data_ptr(), lm.data_ptr(), M, M,
                                                     d_view.data_ptr()),
            "shade_copy": lambda: copy_b.copy_(copy_a),
        }
        wall = {k: [] for k in ops}
        for rnd in range(a.rounds + 1):                      # (round 0: warm-up)
            for k, fn in ops.items():                        # alternated
                t = timed(fn, a.reps)
                if rnd:
                    wall[k].append(t)
        # what the timed calls computed, for the record
        src = torch.zeros(M * M, dtype=torch.int32, device="cuda")
        found = {}
        for rad in (4, 16):
            r.lightmap_dilate_device(lm.data_ptr(), d_mask.data_ptr(), lm_out.data_ptr(), M, M, rad, src.data_ptr())
            found[rad] = float((src >= 0).float().mean())
        f = np.frombuffer(d_feat.cpu().numpy().tobytes(), dtype=pt.FEATURE)
        looked_up = float(((f["prim"] >= 0) & (f["prim"] < nt)).mean())

    med = {k: statistics.median(v) * 1e6 for k, v in wall.items()}
    line = dict(map=M, width=W, height=H, rounds=a.rounds, reps=a.reps, num_tris=nt,
                uncovered_fraction=float(1.0 - mask.mean()), filled_or_covered_r4=found[4], filled_or_covered_r16=found[16],
                view_looked_up_fraction=looked_up,
                dilate_bytes=M * M * 25, view_bytes=n * 60,
                us_median=med, us_min={k: min(v) * 1e6 for k, v in wall.items()},
                us_max={k: max(v) * 1e6 for k, v in wall.items()},
                dilate_r4_over_copy=med["dilate_r4"] / med["dilate_copy"],
                dilate_r16_over_copy=med["dilate_r16"] / med["dilate_copy"],
                shade_over_features=med["shade"] / med["features"], shade_over_copy=med["shade"] / med["shade_copy"])
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
