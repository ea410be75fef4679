"""Glue for the tests of accumulators and feature buffers over caller-supplied rays (include/pt/pt.h,
pt_accum_create_rays*, pt_render_features_rays*).  The references themselves are rays_ref.render (the f64 mean at any
count), noise_ref / adaptive_ref, and the feature restatement of denoise_ref.features_ref with the ray taken from the
buffer instead of pt_camera_ray.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import cudapathtracer_amd as pt

import rays_ref

F = np.float32
W, H, BOUNCES, SEED = 24, 16, 3, 1234

# The adaptive case of tests/test_rays_accum_host.py (its condition, from the restatement) and of
# tests/test_gpu_rays_accum.py: the panorama set (c), passes of 4, cap 32, the project's cornell_blob tolerance.
LOOP = dict(pass_spp=4, cap=32, tol=0.2, quantile=1.0, min_batches=2)


def means(osc, name, o, d, integrator, w=W, h=H):
    """n -> the restatement's (h, w, 3) f64 mean after n samples of every ray of set `name` (cached, read-only)."""
    return lambda n: rays_ref.render_cached("cornell/" + name, osc, o, d, w, h, int(n), BOUNCES, integrator, SEED)[0]


def features_ref(scene_arrays, origins, directions, w, h, trace):
    """The (H, W) FEATURE array of pt_render_features_rays: `trace(origins, directions) -> (tri, t)` of the rays as
    given, then the scene arrays -- denoise_ref.features_ref with the buffer's ray in place of the camera's."""
    o = np.ascontiguousarray(origins, dtype=F).reshape(h, w, 3)
    d = np.ascontiguousarray(directions, dtype=F).reshape(h, w, 3)
    tri, t = trace(o.reshape(-1, 3), d.reshape(-1, 3))
    tri = np.asarray(tri, dtype=np.int32).reshape(h, w)
    t = np.asarray(t, dtype=F).reshape(h, w)
    tris, mats, sph = scene_arrays["tris"], scene_arrays["mats"], scene_arrays["spheres"]
    nt = len(tris)
    f = np.zeros((h, w), dtype=pt.FEATURE)
    f["prim"] = -1
    f["depth"] = t
    for y in range(h):
        for x in range(w):
            k = int(tri[y, x])
            if k < 0:
                continue
            r = f[y, x]
            pos = (o[y, x] + (d[y, x] * t[y, x]).astype(F)).astype(F)
            if k < nt:
                alb, emi = mats[tris[k]["mat"]]["albedo"], mats[tris[k]["mat"]]["emission"]
                nrm = np.array([tris[k]["nx"], tris[k]["ny"], tris[k]["nz"]], dtype=F)
            else:
                s = sph[k - nt]
                alb, emi = s["diffuse"], s["emission"]
                nrm = ((pos - s["pos"].astype(F)).astype(F) / F(s["rad"])).astype(F)
            r["albedo"] = alb.astype(F)
            r["normal"] = nrm
            r["position"] = pos
            r["prim"] = k | (pt.PT_FEATURE_EMISSIVE if emi[0] != 0 else 0)
    return f


def checkerboard(w, h, block=1):
    """(h, w) bool: every other block x block square, starting with the one at (0, 0)."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x // block + y // block) % 2) == 0
