#!/usr/bin/env python3
"""Cost of rendering along caller-supplied rays: the stand-in at 1920x1080, 16 spp.

    python tools/rays_cost.py [--spp 16] [--rounds 5] [--integrator 0] [--accum [--pass-spp 4]] [--out FILE.json]

Alternated in one run, medians over the rounds:
  * render_rays_device on the camera's own rays against render_device of the same camera (the two trace the same rays,
    pixel (0, 0) apart: the difference is the classification launch, the 24 B per pixel the set-up reads and the
    origin read per sample start), with a panorama from the same position beside them;
  * classify_rays_device of the same buffer against a device-to-device copy of its 24 B per ray, the kernel's traffic
    floor (timed with events around each, same stream);
  * at --small-width x --small-height and --small-spp: a buffer with one far ray and one unnormalised direction -- the
    whole render on the tile kernel with the reference's walk -- against the regular buffer it was made from.
With --accum, after those (accumulators and feature buffers over rays, the camera's own rays against the camera):
  * a --pass-spp accumulating pass of a ray accumulator against the camera accumulator's;
  * the same pass over the active list, with about 50% and about 10% of the pixels active (the others masked at 0 samples
    by the same random mask on both sides);
  * features_rays_device against features_device (events around the blocking calls);
  * the create call -- the copy of the buffer and its classification on top of a camera accumulator's allocations --
    against creating the camera accumulator (host wall time of the blocking calls).
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

POS = (0.0, 1.0, 3.0)


def _dev(o, d):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32)).cuda()


def _ratio(num, den):
    per_round = [a / b for a, b in zip(num, den)]
    return dict(of_medians=statistics.median(num) / statistics.median(den), min=min(per_round), max=max(per_round))


def accum_blocks(r, a, cam, d_rays, w, h):
    """The --accum blocks: lines of passes, active-list passes, features and the create call, and their ratios."""
    n = w * h
    make = {"rays": lambda: r.accumulator_rays_device(d_rays.data_ptr(), w, h, 3, a.integrator, 1234),
            "camera": lambda: r.accumulator(cam, w, h, 3, a.integrator, 1234)}
    kinds = ["camera", "rays"]
    lines, ratios = [], {}
    rs = np.random.RandomState(5)
    for label, active in (("all", 1.0), ("half", 0.5), ("tenth", 0.1)):
        mask = rs.uniform(size=(h, w)) >= active                 # the masked pixels
        accs = {k: make[k]() for k in kinds}
        try:
            for k in kinds:
                if mask.any():
                    accs[k].freeze(mask)
                accs[k].add(1)                                   # warm-up: buffers, the active list
            t = {k: dict(seconds=[], kernel_ms=[]) for k in kinds}
            units = {}
            for _ in range(a.rounds):
                for k in kinds:                                  # alternated
                    st = accs[k].add(a.pass_spp)
                    t[k]["seconds"].append(st["seconds"])
                    t[k]["kernel_ms"].append(st["kernel_ms"])
                    units[k] = st["work_units"]
        finally:
            for acc in accs.values():
                acc.close()
        line = dict(block="accum_pass_" + label, integrator=a.integrator, width=w, height=h, pass_spp=a.pass_spp, rounds=a.rounds,
                    active_pixels=int(n - mask.sum()))
        for k in kinds:
            sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
            line[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms, seconds_min=min(t[k]["seconds"]),
                           seconds_max=max(t[k]["seconds"]), work_units=units[k])
        lines.append(line)
        ratios["accum_pass_%s_rays_over_camera" % label] = _ratio(t["rays"]["seconds"], t["camera"]["seconds"])
    # ---- the features kernels
    feat = torch.zeros((n * 48,), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_cam, t_rays = [], []
    r.features_device(cam, feat.data_ptr(), w, h)
    r.features_rays_device(d_rays.data_ptr(), feat.data_ptr(), w, h)
    for _ in range(max(a.rounds, 5) * 2):
        ev[0].record()
        r.features_device(cam, feat.data_ptr(), w, h)
        ev[1].record()
        ev[2].record()
        r.features_rays_device(d_rays.data_ptr(), feat.data_ptr(), w, h)   # (classifies the buffer first)
        ev[3].record()
        torch.cuda.synchronize()
        t_cam.append(ev[0].elapsed_time(ev[1]))
        t_rays.append(ev[2].elapsed_time(ev[3]))
    lines.append(dict(block="features", width=w, height=h, features_ms=statistics.median(t_cam), features_ms_min=min(t_cam),
                      features_rays_ms=statistics.median(t_rays), features_rays_ms_min=min(t_rays),
                      note="events around the blocking calls; features_rays includes the classification of the buffer"))
    ratios["features_rays_over_features"] = _ratio(t_rays, t_cam)
    # ---- the create call
    t_create = {k: [] for k in kinds}
    for k in kinds:
        make[k]().close()
    for _ in range(max(a.rounds, 5)):
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = make[k]()
            t_create[k].append((time.perf_counter() - t0) * 1e3)
            acc.close()
    lines.append(dict(block="create", width=w, height=h, rays_bytes=n * 24,
                      create_rays_ms=statistics.median(t_create["rays"]), create_rays_ms_min=min(t_create["rays"]),
                      create_camera_ms=statistics.median(t_create["camera"]), create_camera_ms_min=min(t_create["camera"]),
                      copy_and_classify_ms=statistics.median(t_create["rays"]) - statistics.median(t_create["camera"]),
                      note="host wall time of the blocking create calls; the difference is the ray copy's allocation, the "
                           "device-to-device copy and the classification"))
    lines.append(dict(ratios=ratios))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--integrator", type=int, default=0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--small-width", type=int, default=256)
    ap.add_argument("--small-height", type=int, default=144)
    ap.add_argument("--small-spp", type=int, default=4)
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--accum", action="store_true")
    ap.add_argument("--pass-spp", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    w, h, n = a.width, a.height, a.width * a.height
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, w, h)
    bufs = {"camera_rays": _dev(*rays.camera_rays(cam)), "panorama_rays": _dev(*rays.panorama_rays(POS, w, h))}
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    lines = []
    with pt.Renderer(s, 0) as r:
        def run(kind, width=w, height=h, spp=a.spp, target=out, buffers=bufs, camera=cam):
            if kind == "plain":
                return r.render_device(camera, target.data_ptr(), width, height, spp, 3, a.integrator, 1234)
            return r.render_rays_device(buffers[kind].data_ptr(), target.data_ptr(), width, height, spp, 3, a.integrator, 1234)

        # ---- the render: plain pinhole, its own rays, a panorama
        kinds = ["plain", "camera_rays", "panorama_rays"]
        for k in kinds:                                       # warm-up: tables, buffers
            run(k, spp=1)
        t = {k: dict(seconds=[], kernel_ms=[]) for k in kinds}
        last = {}
        for _ in range(a.rounds):
            for k in kinds:                                   # alternated
                st = run(k)
                t[k]["seconds"].append(st["seconds"])
                t[k]["kernel_ms"].append(st["kernel_ms"])
                last[k] = dict(rays_traced=st["rays_traced"], rays_reference=st["rays_reference"], work_units=st["work_units"],
                               split_pixels=st["split_pixels"])
        line = dict(block="render", integrator=a.integrator, width=w, height=h, spp=a.spp, rounds=a.rounds,
                    note="seconds: the render's device time (set-up + integration kernel); the classification runs before it "
                         "and is timed in the classify block")
        for k in kinds:
            sec, kms = statistics.median(t[k]["seconds"]), statistics.median(t[k]["kernel_ms"])
            line[k] = dict(seconds=sec, kernel_ms=kms, setup_ms=sec * 1e3 - kms, seconds_min=min(t[k]["seconds"]),
                           seconds_max=max(t[k]["seconds"]), **last[k])
        lines.append(line)

        # ---- classify_rays against a copy of the same bytes
        src = bufs["camera_rays"]
        dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t_cls, t_copy, t_call = [], [], []
        r.classify_rays_device(src.data_ptr(), n)
        dst.copy_(src)
        for _ in range(max(a.rounds, 5) * 4):
            ev[0].record()
            cls = r.classify_rays_device(src.data_ptr(), n)   # (blocking: launch, kernel, 16-byte read-back)
            ev[1].record()
            ev[2].record()
            dst.copy_(src)
            ev[3].record()
            torch.cuda.synchronize()
            t_cls.append(ev[0].elapsed_time(ev[1]))
            t_copy.append(ev[2].elapsed_time(ev[3]))
        lines.append(dict(block="classify", rays=n, bytes=n * 24, classes=cls, classify_call_ms=statistics.median(t_cls),
                          classify_call_ms_min=min(t_cls), copy_ms=statistics.median(t_copy), copy_ms_min=min(t_copy),
                          note="classify_call_ms: events around the blocking call (memsets, kernel, read-back, host sync); "
                               "copy_ms: a device-to-device copy of the same 24 B per ray (reads and writes them)"))

        # ---- an irregular buffer against the regular one, small
        sw, sh = a.small_width, a.small_height
        scam = pt.make_camera(POS, 1.0, 3.0, 0.0, sw, sh)
        o, d = rays.camera_rays(scam)
        o2, d2 = o.copy(), d.copy()
        k = (sh // 2) * sw + sw // 2
        o2[k] = (0.0, 1.0, 1000.0)
        d2[k] = (0.0, 0.0, -1.0)
        d2[k + 1] *= np.float32(2.0)
        sb = {"regular": _dev(o, d), "irregular": _dev(o2, d2)}
        sout = torch.zeros((sh, sw, 3), dtype=torch.float32, device="cuda")
        ti = {kk: [] for kk in sb}
        units = {}
        for kk in sb:
            run(kk, sw, sh, 1, sout, sb, scam)
        for _ in range(a.rounds):
            for kk in sb:
                st = run(kk, sw, sh, a.small_spp, sout, sb, scam)
                ti[kk].append(st["seconds"])
                units[kk] = st["work_units"]
        lines.append(dict(block="irregular", width=sw, height=sh, spp=a.small_spp,
                          regular=dict(seconds=statistics.median(ti["regular"]), work_units=units["regular"]),
                          irregular=dict(seconds=statistics.median(ti["irregular"]), work_units=units["irregular"])))
        lines.append(dict(ratios=dict(
            camera_rays_over_plain=_ratio(t["camera_rays"]["seconds"], t["plain"]["seconds"]),
            panorama_rays_over_plain=_ratio(t["panorama_rays"]["seconds"], t["plain"]["seconds"]),
            classify_over_copy=_ratio(t_cls, t_copy),
            irregular_over_regular=_ratio(ti["irregular"], ti["regular"]))))
        if a.accum:
            lines.extend(accum_blocks(r, a, cam, bufs["camera_rays"], w, h))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
