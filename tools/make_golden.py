#!/usr/bin/env python3
"""Generate tests/golden/* from the REFERENCE's own sources (oracle/_ref/refgen) and the oracle.

Run in the build container (needs /root/reference to build refgen):
    make -C oracle && python tools/make_golden.py

Outputs (all small, committed):
  scenes/models/*.obj|.mtl           fixture scenes authored by cudapathtracer_amd.scenes
  scene_<name>.npz                   verts/tris/mats/lights/bvh + meta from the reference's
                                     loadOBJ (modelLoader.h:125) and buildBVH (BVH.h:443)
  standin.json                       sha256 of the same arrays for the 262K-tri stand-in
  kat_tri.npz / kat_aabb.npz         triIntersect / rayAABBIntersect inputs and reference outputs
  kat_cam.npz / kat_morton.npz       cameraRay / Morton maps
  kat_tone.npz                       PPM tone map (int)(gammaCorrect(normalized(c), 1/2.2) * 255)
  xorwow.npz                         oracle XORWOW streams (regression pin)
  render_*.npz                       oracle f64 mean images for small configs (regression pin)
  kat_trace_<scene>.npz              the reference's own trace() (kernel.cu:107-161, compiled from
                                     /root/reference/kernel.cu by oracle/Makefile) on the ray sets of
                                     tests/raysets.py: (triIndex, t) per ray + per-triangle test[]
                                     counts (kernel.cu:133) summed over the rays

  kat_ppm_morton.npz                 the reference's own PPM loop (kernel.cu:763-778, compiled verbatim:
                                     refgen ppm) over a Morton-indexed imgBuffer_host (64x64 f32 values
                                     incl. 0, huge, inf, NaN): the input buffer and the PPM bytes

  scenes/models/closed.obj|.mtl      a closed box with a ceiling light (the blob is loaded into it): the scene in
                                     which no ray of integrator 1 leaves, so none of its samples is undefined
  integ_*.npz                        the reference's own integrators (kernel.cu:217-515 over the samplers :56-99,
                                     compiled verbatim: refgen radiance) and running mean (:551-552: refgen mean)
                                     from given XORWOW states, per sample, in both sin/cos flavours; sets and file
                                     layout in tests/integrator_ref.py

`python tools/make_golden.py --only trace|ppm|integ` regenerates only the kat_trace_* / kat_ppm_* / integ_* files.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from cudapathtracer_amd import scenes  # noqa: E402
from cudapathtracer_amd.api import MAT, NODE, TRI, VEC3  # noqa: E402
import oracle  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from raysets import bounce_rays, ray_sets  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(GOLD, "scenes")
REFGEN = oracle.REFGEN

# name -> list of (obj, origin, scale, flip)   (kernel.cu:590-599 style load lists)
SCENE_SETS = {
    "cornell": [("models/cornell.obj", (0, 0, 0), 1.0, 0)],
    "cornell_blob": [("models/cornell.obj", (0, 0, 0), 1.0, 0), ("models/blob.obj", (0.35, 0.6, 0.3), 0.75, 0)],
    "quirks": [("models/quirks.obj", (0, 0, 0), 1.0, 0)],
    "blob_flip": [("models/blob.obj", (0.1, -0.2, 0.3), 1.5, 1)],
    "nomtl": [("models/nomtl.obj", (0, 0, 0), 1.0, 0)],
    "quad": [("models/quad.obj", (0, 0, 0), 1.0, 0)],
}

# two triangles only (one emissive quad facing the camera): the render path's tree is a root node with
# two single-triangle leaves (accel_build.cpp never makes the root a leaf)
QUAD_OBJ = ("mtllib quad.mtl\nusemtl panel\nv -1 0 -1\nv 1 0 -1\nv 1 2 -1\nv -1 2 -1\nf 1 2 3\nf 1 3 4\n")
QUAD_MTL = "newmtl panel\nKd 0.6 0.5 0.4\nKe 3 2.5 2\n"

NOMTL_OBJ = ("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nusemtl a\nf 1 2 3\n"
             "mtllib does_not_exist.mtl\nf 2 4 3\nusemtl b\nf 1 2 4\n")


def write_quad():
    os.makedirs(os.path.join(SCENES, "models"), exist_ok=True)
    with open(os.path.join(SCENES, "models", "quad.obj"), "w") as fh:
        fh.write(QUAD_OBJ)
    with open(os.path.join(SCENES, "models", "quad.mtl"), "w") as fh:
        fh.write(QUAD_MTL)


def run_ref(args, cwd=None):
    subprocess.check_call([REFGEN] + [str(a) for a in args], cwd=cwd, stdout=subprocess.DEVNULL)


def ref_scene(tmp, name, loads):
    pre = os.path.join(tmp, name)
    args = ["scene", pre]
    for obj, origin, scale, flip in loads:
        args += [obj, origin[0], origin[1], origin[2], scale, flip]
    run_ref(args, cwd=SCENES)
    meta = open(pre + ".meta.txt").read().split()
    return dict(
        verts=np.fromfile(pre + ".verts.bin", VEC3), tris=np.fromfile(pre + ".tris.bin", TRI),
        mats=np.fromfile(pre + ".mats.bin", MAT), lights=np.fromfile(pre + ".lights.bin", "<u4"),
        bvh=np.fromfile(pre + ".bvh.bin", NODE),
        total_light_area=np.float32(float.fromhex(meta[5])), bvh_depth=np.int32(int(meta[7])))


def kat_tri(tmp, rng):
    n = 6000
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    v0 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    v1 = (v0 + rng.normal(scale=0.7, size=(n, 3))).astype(np.float32)
    v2 = (v0 + rng.normal(scale=0.7, size=(n, 3))).astype(np.float32)
    # aim half of the rays at a point inside the triangle (hits), some exactly at edges/vertices
    k = n // 2
    w = rng.dirichlet([1, 1, 1], size=k)
    w[: k // 8, 2] = 0.0
    w[: k // 8] /= w[: k // 8].sum(1, keepdims=True)
    w[k // 8: k // 4] = [1.0, 0.0, 0.0]
    p = w[:, :1] * v0[:k] + w[:, 1:2] * v1[:k] + w[:, 2:] * v2[:k]
    dd = p - o[:k]
    d[:k] = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)
    # degenerate / parallel / axis-aligned cases
    d[k:k + 200] = np.array([0, 0, 1], np.float32)
    v1[k + 200:k + 400] = v0[k + 200:k + 400]                      # zero-area
    d[k + 400:k + 600] = (v1 - v0)[k + 400:k + 600] / np.linalg.norm((v1 - v0)[k + 400:k + 600], axis=1,
                                                                      keepdims=True)   # parallel to edge
    rec = np.concatenate([o, d, v0, v1, v2], 1).astype(np.float32)
    rec.tofile(os.path.join(tmp, "tri.in"))
    run_ref(["tri", os.path.join(tmp, "tri.in"), os.path.join(tmp, "tri.out")])
    t = np.fromfile(os.path.join(tmp, "tri.out"), "<f4")
    np.savez_compressed(os.path.join(GOLD, "kat_tri.npz"), rec=rec, t=t)


def kat_aabb(tmp, rng):
    n = 6000
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    lo = rng.uniform(-1, 0.5, (n, 3)).astype(np.float32)
    hi = (lo + rng.uniform(0, 1, (n, 3))).astype(np.float32)
    # axis-parallel rays, origins on slab planes (0/0 -> NaN), flat boxes
    d[:600, rng.integers(0, 3, 600)] = 0.0
    d[:300, 0] = 0.0
    o[100:400, 0] = lo[100:400, 0]
    hi[400:800, 1] = lo[400:800, 1]
    d[800:1000] = np.array([0, -1, 0], np.float32)
    d[1000:1100] = np.array([-0.0, 0.0, 1.0], np.float32)
    rec = np.concatenate([o, d, lo, hi], 1).astype(np.float32)
    rec.tofile(os.path.join(tmp, "aabb.in"))
    run_ref(["aabb", os.path.join(tmp, "aabb.in"), os.path.join(tmp, "aabb.out")])
    hit = np.fromfile(os.path.join(tmp, "aabb.out"), "<u1")
    np.savez_compressed(os.path.join(GOLD, "kat_aabb.npz"), rec=rec, hit=hit)


def kat_cam(tmp, rng):
    # radius-0 cameras: lens angle kept in (0, pi/2) so the reference's lens term r*cos, r*sin is +0
    # (with cos/sin < 0 it is -0 and only flips the sign of a zero direction component; in the
    # reference those draws come from the racy state[0], kernel.cu:547).  The last camera has a
    # real lens (compared within 1 ulp: cosf/sinf vs the deterministic kernel sin/cos).
    cams = [((0.0, 1.0, 3.0), 1.0, 3.0, 0.0, 512, 512), ((0.0, 2.6, 13.2), 1.0, 3.0, 0.0, 1920, 1080),
            ((0.5, -1.0, 2.0), 2.0, 1.5, 0.0, 97, 61), ((0.0, 1.0, 3.0), 1.0, 3.0, 0.05, 64, 64)]
    out = {}
    for ci, (pos, dist, focal, radius, w, h) in enumerate(cams):
        camb = np.zeros(8, dtype=np.float32)
        camb[:3] = pos
        camb[3:6] = (dist, focal, radius)
        camb = camb.tobytes()[:24] + np.array([w, h], dtype=np.int32).tobytes()
        n = 4000
        ys = rng.integers(0, h, n)
        xs = rng.integers(0, w, n)
        idx = np.array([scenes_morton(x, y) for x, y in zip(xs, ys)], dtype=np.uint32)
        u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        if radius == 0.0:
            u[:, 1] = rng.uniform(1e-3, 0.24, n).astype(np.float32)
        inb = camb + np.concatenate([idx[:, None].view(np.float32), u], 1).astype(np.float32).tobytes()
        open(os.path.join(tmp, "cam.in"), "wb").write(inb)
        run_ref(["cam", os.path.join(tmp, "cam.in"), os.path.join(tmp, "cam.out")])
        ray = np.fromfile(os.path.join(tmp, "cam.out"), "<f4").reshape(n, 6)
        out["cam%d" % ci] = np.array([*pos, dist, focal, radius, w, h], dtype=np.float64)
        out["idx%d" % ci] = idx
        out["u%d" % ci] = u
        out["ray%d" % ci] = ray
    np.savez_compressed(os.path.join(GOLD, "kat_cam.npz"), **out)


def scenes_morton(x, y):
    r = 0
    for b in range(16):
        r |= ((int(x) >> b) & 1) << (2 * b)
        r |= ((int(y) >> b) & 1) << (2 * b + 1)
    return r


def kat_morton(tmp):
    n = 1 << 16
    run_ref(["morton", os.path.join(tmp, "morton.out"), n])
    m = np.fromfile(os.path.join(tmp, "morton.out"), "<u4").reshape(n, 2)
    np.savez_compressed(os.path.join(GOLD, "kat_morton.npz"), xy=m[:, 0], back=m[:, 1])


def kat_helpers(tmp, rng):
    """getTangent (kernel.cu:44-54) and BRDF (:101-104) from the reference's own code (refgen helpers):
    random unit normals, the axis directions of both signs, ties |n.y| == |n.z| (where getTangent's strict
    '>' picks c2), and the fixture scenes' face normals; random albedos and the scenes' material albedos."""
    n_rand = 4000
    nr = rng.normal(size=(n_rand, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    a = rng.uniform(0.1, 1.0, 200)
    ties = np.stack([rng.uniform(-1, 1, 200), a, a * rng.choice([-1.0, 1.0], 200)], axis=1)
    ties /= np.linalg.norm(ties, axis=1, keepdims=True)
    face = [load_scene_normals(n) for n in ("cornell", "cornell_blob")]
    nrm = np.concatenate([nr, axes, ties] + face).astype(np.float32)
    alb = rng.uniform(0, 1, (len(nrm), 3))
    mats = np.concatenate([np.load(os.path.join(GOLD, "scene_%s.npz" % n))["mats"]["albedo"] for n in ("cornell", "quirks")])
    alb[: len(mats)] = mats
    rec = np.zeros(len(nrm), dtype=[("n", "<f4", (3,)), ("pad", "<f4"), ("alb", "<f8", (3,))])
    rec["n"] = nrm
    rec["alb"] = alb
    rec.tofile(os.path.join(tmp, "helpers.in"))
    run_ref(["helpers", os.path.join(tmp, "helpers.in"), os.path.join(tmp, "helpers.out")])
    out = np.fromfile(os.path.join(tmp, "helpers.out"), dtype=rec.dtype)
    np.savez_compressed(os.path.join(GOLD, "kat_helpers.npz"), normal=nrm, albedo=alb, tangent=out["n"], brdf=out["alb"])


def load_scene_normals(name):
    tris = np.load(os.path.join(GOLD, "scene_%s.npz" % name))["tris"]
    return np.stack([tris["nx"], tris["ny"], tris["nz"]], axis=1).astype(np.float64)


def kat_tone(tmp, rng):
    c = np.concatenate([rng.exponential(1.0, 3000), rng.uniform(0, 1e-3, 300), [0.0, 1e-300, 1.0, 3.0, 1e6, 1e300],
                        rng.uniform(0, 20, 700)]).astype(np.float64)
    c = c[: (len(c) // 3) * 3].reshape(-1, 3)
    c.tofile(os.path.join(tmp, "tone.in"))
    run_ref(["tone", os.path.join(tmp, "tone.in"), os.path.join(tmp, "tone.out")])
    v = np.fromfile(os.path.join(tmp, "tone.out"), "<i4").reshape(-1, 3)
    np.savez_compressed(os.path.join(GOLD, "kat_tone.npz"), c=c, v=v)


def xorwow_fixture():
    subs = [0, 1, 2, 3, 1023, 1 << 20, (1 << 22) - 1]
    out = {"subs": np.array(subs, dtype=np.uint64)}
    for s in subs:
        out["raw_%d" % s] = oracle.xorwow_stream(1234, s, 64)
        out["uni_%d" % s] = oracle.uniform_stream(1234, s, 64)
    np.savez_compressed(os.path.join(GOLD, "xorwow.npz"), **out)


def render_fixtures():
    import cudapathtracer_amd as pt
    cfgs = [("cornell_blob", 32, 32, 4, 3, 0), ("cornell_blob", 32, 32, 4, 3, 1), ("cornell", 24, 16, 3, 8, 0)]
    for name, w, h, spp, bounces, integ in cfgs:
        s = pt.Scene()
        for obj, origin, scale, flip in SCENE_SETS[name]:
            s.load_obj(os.path.join(SCENES, obj), origin, scale, flip, mtl_basepath=os.path.join(SCENES, "models") + "/")
        s.build_bvh()
        osc = oracle.OracleScene(s.arrays())
        cam = oracle.camera((0.0, 1.0, 3.0), 1.0, 3.0, 0.0, w, h)
        img, cnt = oracle.render(osc, cam, w, h, spp, bounces, integ, 1234)
        np.savez_compressed(os.path.join(GOLD, "render_%s_%dx%d_s%d_b%d_i%d.npz" % (name, w, h, spp, bounces, integ)),
                            img=img, traces=np.uint64(cnt["traces"]))


def ref_trace(tmp, rays, loads, cwd):
    """(tri, t, counts) from the reference's trace() on the scene of `loads` (refgen trace)."""
    rin, rout, rcnt = (os.path.join(tmp, "trace." + k) for k in ("in", "out", "cnt"))
    np.ascontiguousarray(rays, dtype=np.float32).tofile(rin)
    args = ["trace", rin, rout, rcnt]
    for obj, origin, scale, flip in loads:
        args += [obj, origin[0], origin[1], origin[2], scale, flip]
    run_ref(args, cwd=cwd)
    res = np.fromfile(rout, "<i4").reshape(-1, 2)
    return res[:, 0].copy(), res[:, 1].copy().view(np.float32), np.fromfile(rcnt, "<u4")


def kat_trace(tmp):
    """trace() goldens: the ray sets of tests/raysets.py plus first-bounce rays off the interior
    set's hits; for the stand-in, camera rays of the bench view and their bounces first."""
    jobs = [(name, SCENE_SETS[name], SCENES, 1024, None) for name in ("cornell", "cornell_blob", "quirks")]
    gen = os.path.join(tmp, "gen_trace")
    p = scenes.write_sponza_standin(gen)
    jobs.append(("standin", [(os.path.relpath(p, gen), (0, 0, 0), 1.0, 0)], gen, 512, p))
    for name, loads, cwd, n, standin in jobs:
        arrs = ref_scene(tmp, name, loads) if standin is None else None
        if standin is not None:
            import cudapathtracer_amd as pt
            s = pt.Scene()
            s.load_obj(standin, mtl_basepath=os.path.dirname(standin) + "/")
            s.build_bvh()
            arrs = s.arrays()
        sets = []
        if standin is not None:
            import cudapathtracer_amd as pt
            c = scenes.SPONZA_STANDIN_CAMERA
            cam = pt.make_camera(c["pos"], c["dist_from_film"], c["focal_length"], 0.0, 1920, 1080)
            idx = np.random.default_rng(9).integers(0, 1920 * 1080, 4 * n)
            cr = [pt.camera_ray(cam, int(i), lens=False) for i in idx]
            sets.append(("camera", np.array([r[0] for r in cr], np.float32), np.array([r[1] for r in cr], np.float32)))
        for k, (o, d) in ray_sets(arrs, n, 5 if standin is None else 11).items():
            sets.append((k, o, d))
        first = sets[0]
        tri0, t0, _ = ref_trace(tmp, np.concatenate([first[1], first[2]], 1), loads, cwd)
        bo, bd = bounce_rays(arrs, first[1], first[2], tri0, t0, 6 if standin is None else 10)
        sets.append(("bounce", bo, bd))
        rays = np.concatenate([np.concatenate([o, d], 1) for _, o, d in sets]).astype(np.float32)
        tri, t, counts = ref_trace(tmp, rays, loads, cwd)
        offs = np.cumsum([0] + [len(o) for _, o, _ in sets]).astype(np.int64)
        np.savez_compressed(os.path.join(GOLD, "kat_trace_%s.npz" % name), rays=rays, tri=tri, t=t, counts=counts,
                            set_names=np.array([k for k, _, _ in sets]), set_offsets=offs)
        print("kat_trace", name, len(rays), "rays,", int((tri >= 0).sum()), "hits,", int(counts.sum()), "tests")


def kat_ppm_morton(tmp):
    """The reference's PPM loop (kernel.cu:763-778) over a Morton-indexed 64x64 imgBuffer_host."""
    rng = np.random.default_rng(763)
    w = h = 64
    buf = (rng.random((w * h, 3)) * rng.choice([0.01, 1.0, 30.0], size=(w * h, 1))).astype(np.float32)
    buf[:8] = [[0, 0, 0], [1e30, 3e38, np.inf], [np.nan, 1, 2], [1e-30, 0.5, 1e-7], [2.0, 0.25, 255.0],
               [0.0123, 0.9, 7.5], [1.0, 1.0, 1.0], [100.0, 1000.0, 1e4]]
    d = os.path.join(tmp, "ppm")
    os.makedirs(d, exist_ok=True)
    ppm = oracle.ref_ppm_imgbuf(buf, w, h, d)
    np.savez_compressed(os.path.join(GOLD, "kat_ppm_morton.npz"), buf=buf, w=w, h=h,
                        ppm=np.frombuffer(ppm, dtype=np.uint8))
    print("kat_ppm_morton", len(ppm), "bytes")


CLOSED_MTL = "newmtl wall\nKd 0.725 0.71 0.68\nnewmtl lamp\nKd 0.78 0.78 0.78\nKe 17 12 4\n"


def write_closed():
    """models/closed.obj|.mtl: a closed box x, z in [-1, 1] x [-1, 3.5], y in [0, 2] (inward normals, the floor first),
    and a ceiling light quad facing -y.  With the blob loaded into it (integrator_ref.LOADS) and the camera of
    integrator_ref.CAMERA inside, no ray of integrator 1 can leave the scene."""
    q = scenes._oriented_quad
    x0, x1, y0, y1, z0, z1 = -1.0, 1.0, 0.0, 2.0, -1.0, 3.5
    quads = [("wall", q([(x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0)], (0, 1, 0))),      # floor
             ("wall", q([(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)], (0, -1, 0))),     # ceiling
             ("wall", q([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], (0, 0, 1))),      # back
             ("wall", q([(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], (0, 0, -1))),     # front
             ("wall", q([(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)], (1, 0, 0))),      # left
             ("wall", q([(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)], (-1, 0, 0))),     # right
             ("lamp", q([(-0.5, 1.98, 0.0), (0.5, 1.98, 0.0), (0.5, 1.98, 1.0), (-0.5, 1.98, 1.0)], (0, -1, 0)))]
    w = scenes._ObjWriter()
    w.raw("mtllib closed.mtl")
    cur = None
    for mat, quad in quads:
        if mat != cur:
            w.raw("usemtl %s" % mat)
            cur = mat
        w.faces(np.array([[0, 1, 2, 3]]), w.verts(quad))
    scenes._write(SCENES, "closed", w.text(), CLOSED_MTL)


def integ_fixtures(tmp):
    """tests/golden/integ_*.npz (layout: tests/integrator_ref.py): the reference's own integrators and running mean
    on every set of integrator_ref.sets(), both flavours.  Asserts the conditions that keep the d2 flag from hiding a
    failure, and prints the counts (DESIGN.md 5 quotes them)."""
    import integrator_ref as ir
    write_closed()
    caller, total, total_flagged, wrong_spp = {}, 0, 0, []
    ref_loads = {k: [("models/" + o, org, sc, fl) for o, org, sc, fl in v] for k, v in ir.LOADS.items()}
    for name in ir.LOADS:
        verts = ref_scene(tmp, "integ_" + name, ref_loads[name])["verts"]
        v = np.stack([verts["x"], verts["y"], verts["z"]], axis=1)
        caller[name] = ir.caller_rays(v, ir.RAYS_W * ir.RAYS_H, np.random.default_rng(sum(name.encode()) + 417),
                                      pad=-0.02 if name == "closed" else 0.1, region=ir.RAY_REGION.get(name))
    for s in ir.sets():
        w, h, spp = s["w"], s["h"], s["spp"]
        if s["kind"] == "camera":
            cam = oracle.camera(ir.CAMERA_POS[s["scene"]], ir.CAMERA["dist_from_film"], ir.CAMERA["focal_length"],
                                ir.CAMERA["radius"], w, h)
            rays = oracle.camera_rays(cam, w, h)
        else:
            rays = caller[s["scene"]]
        state0 = oracle.xorwow_states(s["seed"], ir.morton_grid(w, h))
        out = dict(rays=rays, state0=state0,
                   meta=np.array([w, h, spp, s["seed"], s["integrator"], s["bounces"], s["kind"] == "rays"], np.int64))
        flags = {}
        if s["integrator"] == 1:
            # 4 spp unless that leaves fewer than a third of the pixels without a flagged sample: then 2 (SPP2)
            st, bad4 = state0, np.zeros(w * h, bool)
            for _ in range(4):
                r = oracle.ref_radiance("det", 1, s["bounces"], rays, st, ref_loads[s["scene"]], SCENES, tmp)
                st, bad4 = r["state"], bad4 | (r["flag"] != 0)
            need = 4 if 3 * int((~bad4).sum()) >= w * h else 2
            if need != spp:
                wrong_spp.append((s["scene"], s["kind"], w, h, s["seed"], need))
        for fl in ir.FLAVOURS:
            st = state0
            res = []
            for _ in range(spp):
                r = oracle.ref_radiance(fl, s["integrator"], s["bounces"], rays, st, ref_loads[s["scene"]], SCENES, tmp)
                st = r["state"]
                res.append(r)
            out["colour_" + fl] = np.stack([r["colour"] for r in res], axis=1)
            out["end_" + fl] = np.stack([r["state"] for r in res], axis=1)
            out["mean_" + fl] = oracle.ref_mean(out["colour_" + fl], tmp)
            flags[fl] = (np.stack([r["flag"] for r in res], axis=1).astype(np.uint8),
                         np.stack([r["misses"] for r in res], axis=1))
        # which calls miss depends on the geometry and the directions' hemispheres; the two flavours' directions
        # differ by an ulp at most, but a flag that differed would make "unflagged" ambiguous: flag the union
        out["flag"] = flags["libm"][0] | flags["det"][0]
        out["misses"] = flags["det"][1]
        n, nf = out["flag"].size, int(out["flag"].sum())
        clean = int((out["flag"].sum(axis=1) == 0).sum())
        print("%-46s samples %5d  flagged %5d (%.1f%%)  pixels without a flagged sample %4d of %4d"
              % (s["name"], n, nf, 100.0 * nf / n, clean, w * h))
        if s["integrator"] == 0:
            assert nf == 0, "integrator 0 is never flagged"
        elif s["scene"] == "closed":
            assert nf <= 0.01 * n, "closed scene: at most 1% flagged"
        else:
            assert n - nf >= 0.4 * n, "open scene: at least 40% unflagged (change the rays, not the cap)"
            assert need != spp or 3 * clean >= w * h, "open scene: at least a third of the pixels comparable"
        total += n
        total_flagged += nf
        np.savez_compressed(os.path.join(GOLD, s["name"] + ".npz"), **out)
    assert not wrong_spp, "integrator_ref.SPP2 must name exactly the sets that need 2 spp; (set, spp needed): %r" % wrong_spp
    print("integ fixtures: %d samples per flavour, %d flagged" % (total, total_flagged))


def integ_crafted(tmp):
    """tests/golden/integ_crafted.npz: samples of integrator 1 in the closed scene, built to reach the guards that no
    drawn sample reaches (coverage).  The start STATE is an input of refgen radiance, so a draw can be
    forced: XORWOW's output is v[4] + d, and d is free.
      A  kernel.cu:340 (G == 0) and :379 (G != G, camera side): the camera ray goes straight down onto the floor
         next to the left wall; the bounce's first draw is forced to u1 = 1, so the cosine ray is horizontal
         (castRay.y = sqrt(max(0, 1 - u1)) = 0): dot(norm, dir) = 0 gives G = 0 at :338, and the ray's start is placed
         0.001 / |dir.x| from the wall, where closestT - 0.001 is too small to move the vertex: x[2] == x[3], seg = 0.
      B  kernel.cu:391 (G != G, middle link): the camera ray goes straight up into the light at the very point the
         light path's first vertex was drawn at, from the height at which o.y + (t - 0.001) equals v0.y - 0.001f in
         float: x[3] == x[0], seg = 0, 0 / 0.
    Every candidate is checked in float32 here with the oracle's trace (pinned by kat_trace_*) before it is kept; that
    the reference's text really takes the lines is read off the coverage run, not assumed."""
    import ctypes as C
    import integrator_ref as ir
    F = np.float32
    loads = [("models/" + o, org, sc, fl) for o, org, sc, fl in ir.LOADS["closed"]]
    osc = oracle.OracleScene(ref_scene(tmp, "crafted_closed", loads))
    L = oracle.lib()
    rng = np.random.default_rng(340379391)

    def draws(words, n):
        st = oracle._state(words)
        return [F(L.or_uniform(C.byref(st))) for _ in range(n)]

    def forced(v, k, want):
        """State {d, v} whose k-th output (1-based) is `want`."""
        st = oracle._state([0, *v])
        for _ in range(k):
            out = L.or_xorwow_next(C.byref(st))
        return np.array([(want - out) & 0xFFFFFFFF, *v], dtype=np.uint32)

    def pulled(o, d, t):
        ta = F(np.float64(t) - 0.001)
        return (o + d * ta).astype(F), ta

    recs = []
    # ---- A
    while len(recs) < 2:
        state = forced(rng.integers(1, 2**32, 5, dtype=np.uint64), 6, 0xFFFFFFFF)
        u = draws(state, 7)
        assert u[5] == F(1.0)
        theta = F(2 * 3.14159 * np.float64(u[6]))
        s, c = C.c_float(), C.c_float()
        L.or_sincos(theta, C.byref(s), C.byref(c))
        x, z = F(F(1.0) * F(c.value)), F(F(1.0) * F(s.value))
        ln = np.sqrt(F(F(x * x) + F(0.0)) + F(z * z), dtype=F)
        d2 = np.array([x / ln, 0.0, -z / ln], dtype=F)            # norm (0,1,0): tangent (1,0,0), bitangent (0,0,-1)
        if d2[0] > -0.5:
            continue
        for z0 in (2.5, 2.25, 2.75, 3.0):
            ox0 = F(-1.0 + 0.001 * abs(float(d2[0])))
            for k in range(-6, 7):
                ox = ox0
                for _ in range(abs(k)):
                    ox = np.nextafter(ox, F(1.0 if k > 0 else -2.0))
                o, d = np.array([ox, 0.5, z0], dtype=F), np.array([0.0, -1.0, 0.0], dtype=F)
                x3, _ = pulled(o, d, oracle.trace(osc, o, d)[1])
                tri, t2 = oracle.trace(osc, x3, d2)
                x2, _ = pulled(x3, d2, t2)
                if tri >= 0 and np.array_equal(x2, x3):
                    recs.append((np.concatenate([o, d]), state))
                    break
            else:
                continue
            break
    # ---- B
    a = osc.verts.view(F).reshape(-1, 3)
    tris = osc.tris
    while len(recs) < 4:
        state = np.array([rng.integers(0, 2**32), *rng.integers(1, 2**32, 5, dtype=np.uint64)], dtype=np.uint32)
        u0, u, v = draws(state, 3)
        ra = F(F(osc.c.total_light_area) * u0)
        sel = 12 if 0 < ra < 0.5 else 13
        assert ra != 0.5 and list(osc.lights) == [12, 13]
        if np.float64(F(u + v)) > 1.0:
            u, v = F(np.float64(u) + 2 * (0.5 - np.float64(u))), F(np.float64(v) + 2 * (0.5 - np.float64(v)))
        v0 = a[tris["v0"][sel]]
        a1, a2 = a[tris["v1"][sel]] - v0, a[tris["v2"][sel]] - v0
        x0 = (((v0 + a1 * u).astype(F) + (a2 * v).astype(F)).astype(F) + np.array([0.0, -1.0, 0.0], F) * F(0.001)).astype(F)
        oy = F(1.9)
        for _ in range(4000):
            o, d = np.array([x0[0], oy, x0[2]], dtype=F), np.array([0.0, 1.0, 0.0], dtype=F)
            tri, t = oracle.trace(osc, o, d)
            if tri == sel and np.array_equal(pulled(o, d, t)[0], x0):
                recs.append((np.concatenate([o, d]), state))
                break
            oy = np.nextafter(oy, F(2.0))
    rays = np.stack([r for r, _ in recs]).astype(F)
    states = np.stack([s for _, s in recs]).astype(np.uint32)
    out = dict(rays=rays, state0=states)
    for fl in ir.FLAVOURS:
        r = oracle.ref_radiance(fl, 1, 3, rays, states, loads, SCENES, tmp)
        assert not r["flag"].any(), "crafted samples must be ones the reference defines"
        out["colour_" + fl], out["end_" + fl] = r["colour"], r["state"]
    np.savez_compressed(os.path.join(GOLD, "integ_crafted.npz"), **out)
    print("integ_crafted", len(rays), "samples: 2 for kernel.cu:340 and :379, 2 for :391")


def main():
    if not os.path.exists(REFGEN):
        sys.exit("oracle/_ref/refgen missing: run `make -C oracle` with /root/reference present")
    if not (oracle.ensure_refgen("radiance") and oracle.ensure_refgen("mean")):
        sys.exit("oracle/_ref/refgen lacks the radiance / mean commands and there is no reference tree to rebuild it")
    if sys.argv[1:] == ["--only", "integ"]:
        with tempfile.TemporaryDirectory() as tmp:
            integ_fixtures(tmp)
            integ_crafted(tmp)
        return
    if sys.argv[1:] == ["--only", "trace"]:
        with tempfile.TemporaryDirectory() as tmp:
            kat_trace(tmp)
        return
    if sys.argv[1:] == ["--only", "helpers"]:
        with tempfile.TemporaryDirectory() as tmp:
            kat_helpers(tmp, np.random.default_rng(20261017))
        return
    if sys.argv[1:] == ["--only", "quad"]:
        write_quad()
        with tempfile.TemporaryDirectory() as tmp:
            arrs = ref_scene(tmp, "quad", SCENE_SETS["quad"])
            np.savez_compressed(os.path.join(GOLD, "scene_quad.npz"), **arrs)
            print("scene quad", len(arrs["tris"]), "tris, depth", int(arrs["bvh_depth"]))
        return
    if sys.argv[1:] == ["--only", "ppm"]:
        with tempfile.TemporaryDirectory() as tmp:
            kat_ppm_morton(tmp)
        return
    os.makedirs(GOLD, exist_ok=True)
    if os.path.isdir(SCENES):
        shutil.rmtree(SCENES)
    scenes.write_cornell(SCENES)
    scenes.write_blob(SCENES, level=3)
    scenes.write_quirks(SCENES)
    with open(os.path.join(SCENES, "models", "nomtl.obj"), "w") as fh:
        fh.write(NOMTL_OBJ)
    write_quad()
    rng = np.random.default_rng(20261015)
    with tempfile.TemporaryDirectory() as tmp:
        for name, loads in SCENE_SETS.items():
            arrs = ref_scene(tmp, name, loads)
            np.savez_compressed(os.path.join(GOLD, "scene_%s.npz" % name), **arrs)
            print("scene", name, len(arrs["tris"]), "tris, depth", int(arrs["bvh_depth"]))
        gen = os.path.join(tmp, "gen")
        p = scenes.write_sponza_standin(gen)
        pre = os.path.join(tmp, "standin")
        run_ref(["scene", pre, os.path.relpath(p, gen), 0, 0, 0, 1, 0], cwd=gen)
        digest = {}
        for part in ("verts", "tris", "mats", "lights", "bvh"):
            digest[part] = hashlib.sha256(open("%s.%s.bin" % (pre, part), "rb").read()).hexdigest()
        meta = open(pre + ".meta.txt").read().split()
        digest["meta"] = meta
        digest["obj_sha256"] = hashlib.sha256(open(p, "rb").read()).hexdigest()
        with open(os.path.join(GOLD, "standin.json"), "w") as fh:
            json.dump(digest, fh, indent=1)
        print("standin", meta)
        kat_tri(tmp, rng)
        kat_aabb(tmp, rng)
        kat_cam(tmp, rng)
        kat_morton(tmp)
        kat_tone(tmp, rng)
        kat_helpers(tmp, rng)
        kat_trace(tmp)
        kat_ppm_morton(tmp)
        integ_fixtures(tmp)
        integ_crafted(tmp)
    xorwow_fixture()
    render_fixtures()
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    main()
