#!/usr/bin/env python3
"""Cost of the ray queries on device buffers: the stand-in, 2^22 rays of three kinds, every
variant alternated in one process after a warm-up round.

    python tools/query_cost.py [--log2n 22] [--rounds 5] [--refill 1,8,16,32,48,64] [--out FILE.json]

Ray sets (built on the device from the bench view):
  camera    coherent camera rays: a 2^k x 2^k pixel grid over the film, in 8x8 tiles (a wave = one tile)
  bounce    incoherent first-bounce rays: from the camera rays' hits at t - 0.001, uniform random directions
  shadow    segments from those hits towards uniform points on the emitters, tmax = the distance

Prints one JSON line.  Per set, the device time (events on the stream around the blocking call: the kernel,
nothing else) of
  lockstep        trace_rays<false, false>, pt_trace's kernel, on the same device rays (PT_QUERY_LOCKSTEP=1): the baseline
  query@R         query_rays<false> refilling once R lanes of a wave are idle (PT_QUERY_REFILL; query@64 is the
                  lock-step loop inside query_rays)
and on the shadow set also
  occluded@R      query_rays<true> likewise
as median, min and max over the rounds, in ms and Mrays/s; then the wall time of host pt_trace against
pt_trace_device for n = 2^16 and 2^log2n.  All variants' answers are compared with the baseline's before timing.
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

KNOBS = ("PT_QUERY_LOCKSTEP", "PT_QUERY_REFILL")


def set_knobs(**kw):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        os.environ["PT_QUERY_" + k.upper()] = str(v)


def camera_rays(cam_desc, side):
    """side x side pinhole rays of the bench camera (camera_ray's arithmetic, in torch float32), in 8x8 tiles."""
    i = torch.arange(side * side, device="cuda")
    tile, within = i // 64, i % 64
    px = (tile % (side // 8)) * 8 + within % 8
    py = (tile // (side // 8)) * 8 + within // 8
    dist, focal = cam_desc["dist_from_film"], cam_desc["focal_length"]
    film = torch.stack([px.float() / side - 0.5, py.float() / side - 0.5, torch.full_like(px, dist, dtype=torch.float32)], dim=1)
    d = film * (-focal / dist)
    d = d / d.norm(dim=1, keepdim=True)
    o = torch.tensor(cam_desc["pos"], dtype=torch.float32, device="cuda").expand_as(d)
    return torch.cat([o, d], dim=1).contiguous()


def emitter_points(arrays, n, gen):
    """n uniform points on the emissive triangles (area-weighted), float32 on the device."""
    T, V, M = arrays["tris"], arrays["verts"], arrays["mats"]
    P = np.stack([V["x"], V["y"], V["z"]], axis=1).astype(np.float64)
    em = np.nonzero(M["emission"][T["mat"]].sum(axis=1) > 0)[0]
    a, b, c = P[T["v0"][em]], P[T["v1"][em]], P[T["v2"][em]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    pick = torch.multinomial(torch.tensor(area / area.sum(), dtype=torch.float32, device="cuda"), n, replacement=True, generator=gen)
    u = torch.rand(n, 2, device="cuda", generator=gen)
    su = u[:, 0].sqrt()
    w0, w1, w2 = 1 - su, su * (1 - u[:, 1]), su * u[:, 1]
    ta, tb, tc = (torch.tensor(x, dtype=torch.float32, device="cuda")[pick] for x in (a, b, c))
    return w0[:, None] * ta + w1[:, None] * tb + w2[:, None] * tc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--refill", default="1,8,16,32,48,64")
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "pt_bench_scene"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.log2n % 2 == 0 and a.log2n >= 16
    n, side = 1 << a.log2n, 1 << (a.log2n // 2)
    refills = [int(x) for x in a.refill.split(",")]
    p = os.path.join(a.cache_dir, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(a.cache_dir)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    arrays = s.arrays()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    stream = torch.cuda.Stream()
    tri = torch.zeros(n, dtype=torch.int32, device="cuda")
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    line = dict(n=n, rounds=a.rounds, refill=refills)
    with pt.Renderer(s, 0) as r, torch.cuda.stream(stream):
        def run_trace(rays, **knobs):
            set_knobs(**knobs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r.trace_device(rays.data_ptr(), n, tri.data_ptr(), t.data_ptr(), stream_ptr=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def run_occ(rays, tmax, **knobs):
            set_knobs(**knobs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r.occluded_device(rays.data_ptr(), n, occ.data_ptr(), tmax.data_ptr(), stream_ptr=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        # ---- the ray sets
        cam = camera_rays(scenes.SPONZA_STANDIN_CAMERA, side)
        run_trace(cam, lockstep=1)
        hit = torch.nonzero(tri >= 0).flatten()
        src = hit[torch.arange(n, device="cuda") % len(hit)]          # every ray leaves a hit point
        pos = cam[src, :3] + cam[src, 3:] * (t[src] - 0.001)[:, None]
        d = torch.randn(n, 3, device="cuda", generator=gen)
        bounce = torch.cat([pos, d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()
        seg = emitter_points(arrays, n, gen) - pos
        dist = seg.norm(dim=1)
        shadow = torch.cat([pos, seg / dist[:, None]], dim=1).contiguous()
        sets = dict(camera=cam, bounce=bounce, shadow=shadow)
        line["camera_hit_fraction"] = len(hit) / n

        # ---- the variants, checked against the baseline, then alternated
        variants = {"lockstep": lambda rays: run_trace(rays, lockstep=1)}
        for R in refills:
            variants["query@%d" % R] = lambda rays, R=R: run_trace(rays, refill=R)
        occ_variants = {}
        for R in refills:
            occ_variants["occluded@%d" % R] = lambda rays, R=R: run_occ(rays, dist, refill=R)
        for name, rays in sets.items():
            run_trace(rays, lockstep=1)
            btri, bt = tri.clone(), t.clone()
            for k, f in variants.items():
                f(rays)
                assert torch.equal(tri, btri) and torch.equal(t.view(torch.int32), bt.view(torch.int32)), (name, k)
            if name == "shadow":
                want = ((btri >= 0) & (bt < dist)).to(torch.uint8)
                line["shadow_occluded_fraction"] = float(want.float().mean())
                for k, f in occ_variants.items():
                    f(rays)
                    assert torch.equal(occ, want), (name, k)
        times = {name: {k: [] for k in list(variants) + (list(occ_variants) if name == "shadow" else [])} for name in sets}
        for rnd in range(a.rounds + 1):                     # (round 0: warm-up)
            for name, rays in sets.items():
                for k, f in list(variants.items()) + (list(occ_variants.items()) if name == "shadow" else []):
                    ms = f(rays)
                    if rnd:
                        times[name][k].append(ms)
        for name in sets:
            line[name] = {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v),
                                  mrays_per_s=n / statistics.median(v) / 1e3) for k, v in times[name].items()}

        # ---- host pt_trace against pt_trace_device (wall time; the latter's rays are on the device already)
        set_knobs()
        wall = {}
        for m in (1 << 16, n):
            rays = sets["bounce"][:m].contiguous()
            h = rays.cpu().numpy()
            ho, hd = np.ascontiguousarray(h[:, :3]), np.ascontiguousarray(h[:, 3:])
            th, td = [], []
            for rnd in range(a.rounds + 1):
                t0 = time.perf_counter()
                r.trace(ho, hd)
                t1 = time.perf_counter()
                r.trace_device(rays.data_ptr(), m, tri.data_ptr(), t.data_ptr(), stream_ptr=stream.cuda_stream)
                t2 = time.perf_counter()
                if rnd:
                    th.append(t1 - t0)
                    td.append(t2 - t1)
            wall[str(m)] = dict(host_trace_ms_median=statistics.median(th) * 1e3, trace_device_ms_median=statistics.median(td) * 1e3)
        line["wall"] = wall
    set_knobs()
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
