"""Scenes and ray sets for the light-list and sphere tests (test_light_scenes_host.py, test_gpu_light_scenes.py).

The shading code branches on the number of lights and on the presence of spheres (pt_render.hip: kLdsLights,
kMaxProbeEmitters, num_spheres > 0).  `write_lit_soup` writes a triangle soup with any number of emissive
triangles, `add_random_spheres` appends spheres to a pt.Scene, and the ray sets aim at what sphere code gets
wrong: origins inside spheres, rays leaving surfaces at t - 0.001, silhouettes.  Three restatements are here
too: the sphere test in float32 numpy (the oracle's order of operations), the nearest sphere in plain float64
geometry, and the host's light list and running light area."""
import math
import os

import numpy as np

import raysets

LIGHT_SPHERE = 0x80000000            # PT_LIGHT_SPHERE
MISS_T = np.float32(1e5)             # closestT of a miss (MAX_FLOAT, kernel.cu)
BOX = ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))
SPHERE_RADII = (0.02, 0.15, 0.4)
EMISSIVE_RADII = (0.4, 0.15, 0.08, 0.25, 0.02, 0.3)
SHELL_RADIUS = 6.0
EMISSIVE_MTL = (("e0", (12.0, 11.0, 10.0)), ("e1", (6.0, 9.0, 3.0)), ("e2", (0.5, 0.25, 4.0)))


def _unit(v):
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


# ----------------------------------------------------------------------------- the lit soup

def write_lit_soup(dirpath, seed, n_emissive, first_emissive=None, n_random=150, name="lit"):
    """Write <dirpath>/<name>.obj/.mtl: a random soup with exactly `n_emissive` emissive triangles; returns the
    OBJ path.

    The body: `n_random` random triangles in [-2, 2]^3 (eight of them, and a ninth in front of the standard
    camera, under `cyan`, Ke 0 5 5: emission[0] == 0, so neither a light nor a probe emitter), two fans,
    axis-aligned quads (one the floor y = 0 under add_random_spheres' tangent sphere) and two zero-area triangles.

    The emitters use the materials e0..e2 in turn, have random orientations and areas spread over four decades
    (edge scale 1 down to 0.01), and sit throughout the OBJ order.  `first_emissive` (default: seed is odd) makes
    an emitter triangle 0 -- the record a light pick that selects nothing falls back to -- or keeps triangle 0 a
    plain one.

    With n_emissive >= 3 these are among the emitters (they count towards n_emissive):
      * one zero-area emitter (in the light list with area 0, normal NaN);
      * one emitter 0.01 behind a non-emissive triangle 1.15 times its size (the probe finds the emitter, the
        walk the blocker);
      * an emitter that is an exact copy of a non-emissive triangle listed before it and one that copies a
        non-emissive triangle listed after it (equal t at the probe's bound; the reference's first-visited
        triangle wins).  With n_emissive == 3 there is room for one such emitter only: it then sits between two
        non-emissive copies of itself, one listed before and one after."""
    rng = np.random.default_rng(seed)
    if first_emissive is None:
        first_emissive = seed % 2 == 1
    entries = []                                            # (key in the OBJ order, a, b, c, material)

    def put(key, a, b, c, m):
        entries.append((float(key), np.asarray(a, float), np.asarray(b, float), np.asarray(c, float), m))

    body = []
    for k in range(n_random):
        c = rng.uniform(-2, 2, 3)
        s = rng.choice([0.05, 0.3, 1.0])
        body.append((c + rng.normal(0, s, 3), c + rng.normal(0, s, 3), c + rng.normal(0, s, 3),
                     "cyan" if k % 19 == 7 else "m%d" % rng.integers(3)))
    c = np.array([0.0, 1.0, 0.5])                           # one cyan triangle the standard camera sees
    body.insert(n_random // 2, (c + rng.normal(0, 0.5, 3), c + rng.normal(0, 0.5, 3), c + rng.normal(0, 0.5, 3), "cyan"))
    for f in range(2):                                      # fans: 8 triangles around a shared vertex
        ctr = rng.uniform(-1.5, 1.5, 3)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 9))
        ring = [ctr + 0.6 * np.array([np.cos(t), np.sin(t), 0.2 * np.sin(3 * t)]) for t in ang]
        for j in range(8):
            body.append((ctr, ring[j], ring[j + 1], "m%d" % (j % 3)))
    for ax in range(3):                                     # axis-aligned quads (flat boxes)
        for q in range(2):
            o = rng.uniform(-2, 2, 3)
            e1, e2 = np.zeros(3), np.zeros(3)
            e1[(ax + 1) % 3] = rng.uniform(0.2, 1.0)
            e2[(ax + 2) % 3] = rng.uniform(0.2, 1.0)
            if ax == 1 and q == 0:                          # the floor
                o, e1, e2 = np.array([-1.0, 0.0, -1.0]), np.array([0.0, 0.0, 2.0]), np.array([2.0, 0.0, 0.0])
            body.append((o, o + e1, o + e1 + e2, "m0"))
            body.append((o, o + e1 + e2, o + e2, "m1"))
    for _ in range(2):                                      # zero-area triangles
        p, q = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        body.append((p, q, p + 0.5 * (q - p), "m2"))
    for k, (a, b, c, m) in enumerate(body):
        put(k / len(body), a, b, c, m)                      # keys 0 .. < 1

    def big():
        c = np.array([rng.uniform(-0.8, 0.8), rng.uniform(1.0, 2.0), rng.uniform(-0.8, 0.8)])
        return c + rng.normal(0, 0.8, 3), c + rng.normal(0, 0.8, 3), c + rng.normal(0, 0.8, 3)

    emitters = []                                           # (key, a, b, c): the materials follow the final order
    n_special = 0 if n_emissive < 3 else (3 if n_emissive == 3 else 4)
    n_regular = n_emissive - n_special
    for k in range(n_regular):
        c = rng.uniform(-1.5, 1.5, 3) + np.array([0.0, 0.5, 0.0])
        s = 10.0 ** (-2.0 * k / max(n_regular - 1, 1))      # areas ~ s^2: four decades
        key = -1.0 if (k == 0 and first_emissive) else rng.uniform(0.02, 0.98)
        emitters.append((key, c + rng.normal(0, s, 3), c + rng.normal(0, s, 3), c + rng.normal(0, s, 3)))
    if n_special:
        p, q = np.round(rng.uniform(-1, 1, (2, 3)) * 64) / 64                     # (exact in float32, and so
        emitters.append((0.45, p, q, p + 0.25 * (q - p)))                          # is the third point): zero area
        a, b, c = big()                                                             # occluded
        nrm = np.cross(b - a, c - a)
        nrm /= np.linalg.norm(nrm)
        g = (a + b + c) / 3.0
        put(0.2, *(g + 1.15 * (v - g) + 0.01 * nrm for v in (a, b, c)), "m1")
        emitters.append((-1.0 if (n_regular == 0 and first_emissive) else 0.7, a, b, c))
        if n_special == 3:                                                          # copy, emitter, copy
            a, b, c = big()
            put(0.1, a, b, c, "m0")
            emitters.append((0.5, a, b, c))
            put(0.9, a, b, c, "m2")
        else:
            a, b, c = big()
            put(0.1, a, b, c, "m0")
            emitters.append((0.6, a, b, c))                                         # copy of an earlier triangle
            a, b, c = big()
            emitters.append((0.3, a, b, c))                                         # copy of a later triangle
            put(0.9, a, b, c, "m2")
    assert len(emitters) == n_emissive
    for k, (key, a, b, c) in enumerate(sorted(emitters, key=lambda e: e[0])):
        put(key, a, b, c, EMISSIVE_MTL[k % len(EMISSIVE_MTL)][0])
    entries.sort(key=lambda e: e[0])                        # (stable)

    obj, cur, nv = ["mtllib %s.mtl" % name], None, 0
    for _, a, b, c, m in entries:
        if m != cur:
            obj.append("usemtl " + m)
            cur = m
        obj += ["v %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in (a, b, c)]
        obj.append("f %d %d %d" % (nv + 1, nv + 2, nv + 3))
        nv += 3
    mtl = []
    for k, kd in enumerate(rng.uniform(0.2, 0.9, (3, 3))):
        mtl += ["newmtl m%d" % k, "Kd %.6g %.6g %.6g" % tuple(kd)]
    mtl += ["newmtl cyan", "Kd 0.3 0.6 0.6", "Ke 0 5 5"]
    for nm, ke in EMISSIVE_MTL:
        mtl += ["newmtl " + nm, "Kd 0.8 0.8 0.8", "Ke %g %g %g" % ke]
    os.makedirs(dirpath, exist_ok=True)
    with open(os.path.join(dirpath, name + ".mtl"), "w") as fh:
        fh.write("\n".join(mtl) + "\n")
    path = os.path.join(dirpath, name + ".obj")
    with open(path, "w") as fh:
        fh.write("\n".join(obj) + "\n")
    return path


# ----------------------------------------------------------------------------- spheres

def add_random_spheres(scene, seed, n, n_emissive, shell=False, sphere0_emissive=False, box=BOX,
                       radii=SPHERE_RADII):
    """Append `n` spheres to a pt.Scene; returns their (pos, rad, diffuse, emission) list in add order.

    Radii come from `radii` and the centres lie inside `box`, so many spheres overlap.  Sphere 1 touches the
    plane y = 0 (centre height = radius).  The last two spheres (one when n < 6, none when n < 3) are exact
    copies of earlier ones under another colour: the first listed must win every tie.  `n_emissive` of the others
    emit, each with another radius (EMISSIVE_RADII) and its centre in the inner half of the box: the
    highest-numbered ones, and sphere 0 first if `sphere0_emissive`.  With `shell`, sphere 0 is a diffuse sphere of radius 6 around the box, so every camera
    and every ray origin lies inside a sphere."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(box[0], float), np.asarray(box[1], float)
    n_dup = 2 if n >= 6 else (1 if n >= 3 else 0)
    n_base = n - n_dup
    cand = ([0] if sphere0_emissive else []) + list(range(n_base - 1, 0, -1))
    emis = cand[:n_emissive]
    if len(emis) < n_emissive:
        raise ValueError("add_random_spheres: no room for %d emissive spheres among %d" % (n_emissive, n))
    out = []
    for k in range(n_base):
        pos = rng.uniform(lo, hi)
        rad = float(rng.choice(radii))
        col = tuple(float(v) for v in rng.uniform(0.2, 0.9, 3))
        emm = (0.0, 0.0, 0.0)
        if k in emis:                                       # in the inner half of the box
            j = emis.index(k)
            pos = 0.5 * (lo + hi) + 0.5 * (pos - 0.5 * (lo + hi))
            rad = EMISSIVE_RADII[j % len(EMISSIVE_RADII)] * (radii[-1] / SPHERE_RADII[-1])
            emm = ((8.0, 7.0, 6.0), (3.0, 6.0, 9.0), (5.0, 2.0, 1.0))[j % 3]
        if k == 0 and shell:
            pos, rad = 0.5 * (lo + hi), SHELL_RADIUS
        if k == 1:                                          # tangent to y = 0 (the same float32 twice)
            rad = float(np.float32(rad))
            pos = np.array([0.4 * pos[0], rad, 0.4 * pos[2]])
        out.append((tuple(float(v) for v in pos), rad, col, emm))
    first = 1 if shell else 0
    for j in range(n_dup):                                  # copies of earlier spheres, plain and recoloured
        src = out[(first + n_base // 2) % n_base] if j == 0 else out[min(1, n_base - 1)]
        out.append((src[0], src[1], tuple(float(v) for v in rng.uniform(0.2, 0.9, 3)), (0.0, 0.0, 0.0)))
    for pos, rad, col, emm in out:
        scene.add_sphere(pos, rad, col, emm)
    return out


def _centres(spheres):
    return spheres["pos"].astype(np.float64), spheres["rad"].astype(np.float64)


def sphere_ray_sets(spheres, n, seed, box=BOX):
    """Dict of named (origins, directions) float32 arrays for a scene's `spheres` (arrays()["spheres"]):
    interior  origins uniform in `box`, uniform directions;
    inside    origins inside spheres (each sphere in turn, the point uniform in its ball);
    grazing   origins in `box`, aimed along the tangent cone of a sphere they lie outside of -- at its silhouette,
              where hit or miss turns on the sign of the rounded discriminant."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(box[0], float), np.asarray(box[1], float)
    C, R = _centres(spheres)
    out = {}
    o = rng.uniform(lo, hi, (n, 3))
    out["interior"] = (o.astype(np.float32), _unit(rng.normal(size=(n, 3))))
    k = np.arange(n) % len(C)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    rho = 0.999 * rng.uniform(0, 1, n) ** (1.0 / 3.0)
    out["inside"] = ((C[k] + u * (R[k] * rho)[:, None]).astype(np.float32), _unit(rng.normal(size=(n, 3))))
    og = rng.uniform(lo, hi, (n, 3))
    k = rng.integers(len(C), size=n)
    oc = C[k] - og
    L = np.linalg.norm(oc, axis=1)
    w = np.cross(oc, rng.normal(size=(n, 3)))               # a random direction perpendicular to oc
    w /= np.maximum(np.linalg.norm(w, axis=1), 1e-30)[:, None]
    sin_a = np.minimum(R[k] / np.maximum(L, 1e-30), 1.0)    # (an origin inside the sphere: aim across it)
    d = oc / np.maximum(L, 1e-30)[:, None] * np.sqrt(1.0 - sin_a ** 2)[:, None] + w * sin_a[:, None]
    out["grazing"] = (og.astype(np.float32), _unit(d))
    return out


def leaving_rays(trace, o, d, seed):
    """Rays leaving the surfaces that (o, d) hit, as the integrator builds them (raysets.bounce_rays:
    origin o + d * (t - 0.001)); `trace` maps (o, d) to (prim, t)."""
    tri, t = trace(o, d)
    return raysets.bounce_rays(None, o, d, tri, t, seed)


# ----------------------------------------------------------------------------- restatements

def sphere_trace_f32(spheres, o, d, tri0, t0, num_tris):
    """trace() with spheres, restated in float32 numpy: starting from the triangle walk's (tri0, t0), every
    sphere in order replaces the hit if its root is nearer (strict <, so triangles and earlier spheres keep
    ties).  The root, in float and in this order: oc = o - c, b = oc.d, c = oc.oc - r*r, disc = b*b - c; a
    miss unless disc >= 0; -b - sqrt(disc) if > 0, else -b + sqrt(disc) if > 0, else a miss.  Returns (prim, t)."""
    f = np.float32
    o = np.ascontiguousarray(o, dtype=f)
    d = np.ascontiguousarray(d, dtype=f)
    bi = np.array(tri0, dtype=np.int32, copy=True)
    bt = np.array(t0, dtype=f, copy=True)
    for k, sp in enumerate(spheres):
        oc = o - sp["pos"].astype(f)[None, :]
        b = (oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1]) + oc[:, 2] * d[:, 2]
        cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - f(sp["rad"]) * f(sp["rad"])
        disc = b * b - cc
        assert b.dtype == f and cc.dtype == f and disc.dtype == f
        ok = disc >= 0
        q = np.sqrt(np.where(ok, disc, f(0)))
        ts = -b - q
        far = -b + q
        ts = np.where(ts > 0, ts, far)
        ok &= ts > 0
        take = ok & (ts < bt)
        bt = np.where(take, ts, bt).astype(f)
        bi = np.where(take, np.int32(num_tris + k), bi).astype(np.int32)
    return bi, bt


def sphere_nearest_f64(spheres, o, d, eps=1e-3):
    """The nearest sphere along each ray in plain float64 geometry: the positive roots of |o + t d - c|^2 = r^2
    (with a = d.d, not assumed 1).  Exact copies of an earlier sphere are the same surface and count once, under
    the first listed id.  Returns (id or -1, t or 1e5, ambiguous): `ambiguous` marks the rays where float32
    cannot be asked for the same answer at the scale eps -- the two smallest positive roots over all spheres lie
    within eps of each other, or some root lies within eps of 0."""
    o = np.asarray(o, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    C, R = _centres(spheres)
    seen, first = {}, []
    for k in range(len(C)):
        key = (C[k].tobytes(), R[k].tobytes())
        if key not in seen:
            seen[key] = k
            first.append(k)
    n = len(o)
    a = np.einsum("ij,ij->i", d, d)
    roots = np.full((n, 2 * len(first)), np.inf)
    near0 = np.zeros(n, dtype=bool)
    for j, k in enumerate(first):
        oc = o - C[k]
        hb = np.einsum("ij,ij->i", oc, d)
        c = np.einsum("ij,ij->i", oc, oc) - R[k] * R[k]
        disc = hb * hb - a * c
        ok = disc >= 0
        q = np.sqrt(np.where(ok, disc, 0.0))
        for s, col in ((-1.0, 2 * j), (1.0, 2 * j + 1)):
            t = (-hb + s * q) / a
            near0 |= ok & (np.abs(t) < eps)
            roots[:, col] = np.where(ok & (t > 0), t, np.inf)
    order = np.argsort(roots, axis=1)[:, :2]
    t1 = roots[np.arange(n), order[:, 0]]
    t2 = roots[np.arange(n), order[:, 1]]
    hit = np.isfinite(t1)
    ids = np.where(hit, np.asarray(first)[order[:, 0] // 2], -1).astype(np.int32)
    ambiguous = near0 | (hit & (t2 - t1 < eps))
    return ids, np.where(hit, t1, float(MISS_T)), ambiguous


def light_list_ref(arrays):
    """The host's light list and running light area restated from the scene arrays: the triangles whose
    material has emission[0] != 0 in triangle order, then PT_LIGHT_SPHERE | k for the emissive spheres in
    add order; total_light_area is the float32 running sum, in that order, of length(cross(v1 - v0, v2 - v0)) / 2
    and 4 * 3.14159f * r * r (left to right), every operation rounded to float32.  Returns (lights, area)."""
    f = np.float32
    tris, mats, v = arrays["tris"], arrays["mats"], arrays["verts"]
    P = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(f)
    lights, total = [], f(0)
    for i in np.nonzero(mats["emission"][tris["mat"], 0] != 0)[0] if len(tris) else []:
        a, b, c = P[tris["v0"][i]], P[tris["v1"][i]], P[tris["v2"][i]]
        p, q = b - a, c - a
        x = f(f(p[1] * q[2]) - f(p[2] * q[1]))
        y = f(f(p[2] * q[0]) - f(p[0] * q[2]))
        z = f(f(p[0] * q[1]) - f(p[1] * q[0]))
        area = f(f(math.sqrt(f(f(f(x * x) + f(y * y)) + f(z * z)))) / f(2))
        total = f(total + area)
        lights.append(int(i))
    for k, sp in enumerate(arrays["spheres"]):
        if sp["emission"][0] != 0:
            r = f(sp["rad"])
            total = f(total + f(f(f(f(4.0) * f(3.14159)) * r) * r))
            lights.append(LIGHT_SPHERE | k)
    return np.array(lights, dtype=np.uint32), total
