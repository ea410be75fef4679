#!/usr/bin/env python3
"""Cost of an irradiance render: the stand-in at 1920x1080, 16 spp, both integrators.

    python tools/irradiance_cost.py [--spp 16] [--rounds 5] [--integrators 0,1] [--accum [--pass-spp 4]] [--out FILE.json]

The points are feature_points of the stand-in's camera: what it sees, lifted 1e-3.  Alternated in one run, medians over
the rounds, per integrator:
  * render_irradiance_device over those points (a pair and a cosine direction per sample, 24 B read per sample start);
  * render_rays_device over the same points with their normals as directions -- the fixed-ray source, whose primary-hit
    memo traces each pixel's ray once;
  * the plain render of the same camera with radius = 0.05, which also forms a ray per sample (a lens pair, no memo);
and once:
  * classify_points_device of the buffer on its own against a device-to-device copy of its 24 B per point (events around
    the blocking calls).
With --accum, after those (accumulators over points, pt_accum_create_points*), per integrator:
  * a --pass-spp accumulating pass of a point accumulator against render_irradiance_device at --pass-spp over the same
    points (the existing one-shot path: the same samples, without the stored mean and stream);
  * the same pass over the active list, with about 50% and about 10% of the pixels active (the others masked at 0
    samples), against the same fractions of a camera accumulator with radius = 0.05 -- the other source whose every
    unit is a lens unit;
  * the add_adaptive loop over the points (--adaptive-tol, --adaptive-cap, passes of --pass-spp, the camera's misses
    masked at 0 samples): samples_total over texels x cap, the saving against uniform sampling to the cap;
and once:
  * the create call against accumulator_rays_device over the same buffer (host wall time of the blocking calls: both
    copy and classify 24 B per pixel).
Prints one JSON line per block and one of ratios, each ratio with the smallest and largest per-round ratio beside the
ratio of the medians.  --out also keeps the lines in a file.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudapathtracer_amd as pt  # noqa: E402
from cudapathtracer_amd import rays, scenes  # noqa: E402


def _ratio(num, den):
    per_round = [a / b for a, b in zip(num, den)]
    return dict(of_medians=statistics.median(num) / statistics.median(den), min=min(per_round), max=max(per_round))


def accum_blocks(r, a, lens_cam, buf, miss, out, w, h):
    """The --accum blocks: lines of passes, active-list passes, the adaptive loop and the create call, and their ratios."""
    n = w * h
    lines, ratios = [], {}
    for integrator in [int(v) for v in a.integrators.split(",")]:
        make = {"points": lambda: r.accumulator_points_device(buf.data_ptr(), w, h, 3, integrator, 1234),
                "lens": lambda: r.accumulator(lens_cam, w, h, 3, integrator, 1234)}
        rs = np.random.RandomState(5)
        for label, active in (("all", 1.0), ("half", 0.5), ("tenth", 0.1)):
            mask = rs.uniform(size=(h, w)) >= active             # the masked pixels
            kinds = ["points", "one_shot"] if label == "all" else ["lens", "points"]
            accs = {k: make[k]() for k in kinds if k != "one_shot"}
            try:
                for acc in accs.values():
                    if mask.any():
                        acc.freeze(mask)
                    acc.add(1)                                   # warm-up: buffers, the active list
                r.render_irradiance_device(buf.data_ptr(), out.data_ptr(), w, h, 1, 3, integrator, 1234)
                t = {k: dict(seconds=[], kernel_ms=[]) for k in kinds}
                units, traced = {}, {}
                for _ in range(a.rounds):
                    for k in kinds:                              # alternated
                        if k == "one_shot":
                            st = r.render_irradiance_device(buf.data_ptr(), out.data_ptr(), w, h, a.pass_spp, 3, integrator, 1234)
                        else:
                            st = accs[k].add(a.pass_spp)
                        t[k]["seconds"].append(st["seconds"])
                        t[k]["kernel_ms"].append(st["kernel_ms"])
                        units[k] = st["work_units"]
                        traced[k] = st["rays_traced"]
            finally:
                for acc in accs.values():
                    acc.close()
            line = dict(block="accum_pass_" + label, integrator=integrator, width=w, height=h, pass_spp=a.pass_spp,
                        rounds=a.rounds, active_pixels=int(n - mask.sum()))
            for k in kinds:
                sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
                line[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms, seconds_min=min(t[k]["seconds"]),
                               seconds_max=max(t[k]["seconds"]), work_units=units[k], rays_traced=traced[k])
            lines.append(line)
            ratios["i%d_accum_pass_%s_points_over_%s" % (integrator, label, kinds[1] if label == "all" else "lens")] = \
                _ratio(t["points"]["seconds"], t["one_shot" if label == "all" else "lens"]["seconds"])
        # ---- the adaptive loop: what a bake saves against uniform sampling to the cap
        texels = int(n - miss.sum())
        with make["points"]() as acc:
            if miss.any():
                acc.freeze(miss.reshape(h, w))                   # (the camera's misses belong to no surface: masked)
            t0 = time.perf_counter()
            res = acc.add_adaptive(a.pass_spp, a.adaptive_cap, tol=a.adaptive_tol, quantile=1.0, min_batches=2)
            wall = time.perf_counter() - t0
        lines.append(dict(block="adaptive", integrator=integrator, width=w, height=h, pass_spp=a.pass_spp, cap=a.adaptive_cap,
                          tol=a.adaptive_tol, texels=texels, masked=int(miss.sum()), passes=res["passes"],
                          stopped_converged=res["stopped_converged"], active=res["active"], samples_total=res["samples_total"],
                          fraction_of_uniform=res["samples_total"] / float(texels * a.adaptive_cap), wall_seconds=wall))
    # ---- the create call, against a ray accumulator over the same bytes
    make = {"points": lambda: r.accumulator_points_device(buf.data_ptr(), w, h, 3, 0, 1234),
            "rays": lambda: r.accumulator_rays_device(buf.data_ptr(), w, h, 3, 0, 1234)}
    t_create = {k: [] for k in make}
    for k in make:
        make[k]().close()
    for _ in range(max(a.rounds, 5)):
        for k in make:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = make[k]()
            t_create[k].append((time.perf_counter() - t0) * 1e3)
            acc.close()
    lines.append(dict(block="create", width=w, height=h, bytes=n * 24,
                      create_points_ms=statistics.median(t_create["points"]), create_points_ms_min=min(t_create["points"]),
                      create_rays_ms=statistics.median(t_create["rays"]), create_rays_ms_min=min(t_create["rays"]),
                      note="host wall time of the blocking create calls over the same buffer, read as points and as rays"))
    ratios["create_points_over_rays"] = _ratio(t_create["points"], t_create["rays"])
    lines.append(dict(ratios=ratios))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--integrators", default="0,1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--accum", action="store_true")
    ap.add_argument("--pass-spp", type=int, default=4)
    ap.add_argument("--adaptive-tol", type=float, default=0.2)
    ap.add_argument("--adaptive-cap", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    w, h, n = a.width, a.height, a.width * a.height
    c = scenes.SPONZA_STANDIN_CAMERA
    cam = pt.make_camera(c["pos"], c["dist_from_film"], c["focal_length"], 0.0, w, h)
    lens_cam = pt.make_camera(c["pos"], c["dist_from_film"], c["focal_length"], 0.05, w, h)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    lines, ratios = [], {}
    with pt.Renderer(s, 0) as r:
        pts, nrm, miss = rays.feature_points(r.features(cam, w, h), 1e-3)
        buf = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, nrm], axis=1), dtype=np.float32)).cuda()

        def run(kind, integrator, spp):
            if kind == "lens":
                return r.render_device(lens_cam, out.data_ptr(), w, h, spp, 3, integrator, 1234)
            call = r.render_irradiance_device if kind == "irradiance" else r.render_rays_device
            return call(buf.data_ptr(), out.data_ptr(), w, h, spp, 3, integrator, 1234)

        kinds = ["irradiance", "fixed_rays", "lens"]
        for integrator in [int(v) for v in a.integrators.split(",")]:
            for k in kinds:                                   # warm-up: tables, buffers
                run(k, integrator, 1)
            t = {k: dict(seconds=[], kernel_ms=[]) for k in kinds}
            last = {}
            for _ in range(a.rounds):
                for k in kinds:                               # alternated
                    st = run(k, integrator, a.spp)
                    t[k]["seconds"].append(st["seconds"])
                    t[k]["kernel_ms"].append(st["kernel_ms"])
                    last[k] = dict(rays_traced=st["rays_traced"], rays_reference=st["rays_reference"],
                                   work_units=st["work_units"], split_pixels=st["split_pixels"])
            line = dict(block="render", integrator=integrator, width=w, height=h, spp=a.spp, rounds=a.rounds,
                        missed_pixels=int(miss.sum()),
                        note="seconds: the render's device time (set-up + integration kernel); the classification runs before "
                             "it and is timed in the classify block")
            for k in kinds:
                sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
                line[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms, seconds_min=min(t[k]["seconds"]),
                               seconds_max=max(t[k]["seconds"]), **last[k])
            lines.append(line)
            ratios["i%d_irradiance_over_fixed_rays" % integrator] = _ratio(t["irradiance"]["seconds"], t["fixed_rays"]["seconds"])
            ratios["i%d_irradiance_over_lens" % integrator] = _ratio(t["irradiance"]["seconds"], t["lens"]["seconds"])

        # ---- classify_points on its own, against a copy of the same bytes
        dst = torch.empty_like(buf)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t_cls, t_copy = [], []
        r.classify_points_device(buf.data_ptr(), n)
        dst.copy_(buf)
        for _ in range(max(a.rounds, 5) * 4):
            ev[0].record()
            cls = r.classify_points_device(buf.data_ptr(), n)   # (blocking: memsets, kernel, 16-byte read-back)
            ev[1].record()
            ev[2].record()
            dst.copy_(buf)
            ev[3].record()
            torch.cuda.synchronize()
            t_cls.append(ev[0].elapsed_time(ev[1]))
            t_copy.append(ev[2].elapsed_time(ev[3]))
        lines.append(dict(block="classify", points=n, bytes=n * 24, classes=cls, classify_call_ms=statistics.median(t_cls),
                          classify_call_ms_min=min(t_cls), copy_ms=statistics.median(t_copy), copy_ms_min=min(t_copy),
                          note="classify_call_ms: events around the blocking call (memsets, kernel, read-back, host sync); "
                               "copy_ms: a device-to-device copy of the same 24 B per point"))
        ratios["classify_over_copy"] = _ratio(t_cls, t_copy)
        lines.append(dict(ratios=ratios))
        if a.accum:
            lines.extend(accum_blocks(r, a, lens_cam, buf, miss, out, w, h))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
