"""Shared by tools/make_golden.py and the integrator tests (test_integrator_host.py, test_gpu_integrator_ref.py):
the scenes, the sets and the file layout of tests/golden/integ_*.npz -- samples of the REFERENCE's own integrators
(refgen radiance: kernel.cu:217-515 over the samplers :56-99, compiled verbatim) and its running mean (refgen mean:
:551-552) from given XORWOW stream states.

One file per set.  Arrays (P = W*H pixels in scanline order y*W + x, S = spp):
  rays         float32 (P, 6)     {o, d}: the oracle's radius-0 camera rays, or the caller's rays of a "rays" set
  state0       uint32  (P, 6)     {d, v[5]} = or_xorwow_init(seed, morton(x, y)); sample s starts where s-1 ended
  colour_<f>   float64 (P, S, 3)  per-sample colour, flavour f = libm (glibc cosf/sinf) or det (or_sincos)
  end_<f>      uint32  (P, S, 6)  stream state after the sample
  flag         uint8   (P, S)     1 = "reference undefined (d2)": integrator 1's camera bounce missed and the reference
                                  read tris[-1] (kernel.cu:336, 345-346; refgen supplies a sentinel there)
  misses       uint32  (P, S)     bit k set = the sample's k-th trace call missed
  mean_<f>     float64 (P, 3)     refgen mean over the S colours
  meta         int64   (7,)       W, H, S, seed, integrator, bounces, is_rays
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MODELS = os.path.join(GOLD, "scenes", "models")

# (obj, origin, scale, flip) load lists, as kernel.cu:590-599 calls loadOBJ.  `closed` is this module's own: a closed
# box with a ceiling light and the blob inside, so that no ray of integrator 1 leaves the scene.
LOADS = {
    "closed": [("closed.obj", (0, 0, 0), 1.0, 0), ("blob.obj", (0.0, 0.95, 0.3), 0.75, 0)],     # wholly inside
    "cornell_blob": [("cornell.obj", (0, 0, 0), 1.0, 0), ("blob.obj", (0.35, 0.6, 0.3), 0.75, 0)],
    "quirks": [("quirks.obj", (0, 0, 0), 1.0, 0)],
    "blob_flip": [("blob.obj", (0.1, -0.2, 0.3), 1.5, 1)],      # no lights: selectedTri stays 0
}
CAMERA = dict(dist_from_film=1.0, focal_length=3.0, radius=0.0)
# Pinhole camera positions.  (0, 1, 3) is the reference's (kernel.cu:642-648), inside the closed box.  The two small
# open scenes are seen from where integrator 1 stays defined on most samples (its camera bounce must hit something):
# from the reference's position 87% of the quirks samples were flagged.
CAMERA_POS = {"closed": (0.0, 1.0, 3.0), "cornell_blob": (0.0, 1.0, 3.0), "quirks": (2.88, -0.78, 0.15),
              "blob_flip": (0.1, -0.2, 3.5)}
FLAVOURS = ("libm", "det")
SEED_B = 77
RAYS_W, RAYS_H = 16, 12
MODES = ((0, 1), (0, 2), (0, 3), (0, 8), (1, 3))     # (integrator, depth); integrator 1 has no depth


CAMERA_CONFIGS = ((24, 16, 1234), (24, 16, SEED_B), (20, 13, 1234), (20, 13, SEED_B))   # sizes x seeds, crossed
# 4 spp everywhere, except in the integrator-1 sets named here (scene, kind, w, h, seed): there 4 spp leave fewer than
# a third of the pixels without a flagged sample, and the set holds 2.  make_golden.py draws 4 samples for every
# integrator-1 set and asserts that this list is exactly the sets that need it.
SPP2 = {("cornell_blob", "camera", w, h, seed) for w, h, seed in CAMERA_CONFIGS}


def sets():
    """Every fixture set: dict(name, scene, kind, w, h, spp, seed, integrator, bounces).  Every scene at integrator 0
    depths 1, 2, 3 and 8 and at integrator 1, on camera rays at 24x16 and 20x13 with seeds 1234 and 77 (all four
    combinations) and on one buffer of caller rays per scene (16x12, seed 1234)."""
    out = []
    for scene in LOADS:
        for kind, w, h, seed in [("camera",) + c for c in CAMERA_CONFIGS] + [("rays", RAYS_W, RAYS_H, 1234)]:
            for integ, bounces in MODES:
                spp = 2 if (integ == 1 and (scene, kind, w, h, seed) in SPP2) else 4
                name = "integ_%s_%s_%dx%d_s%d_i%d_b%d" % (scene, kind, w, h, seed, integ, bounces)
                out.append(dict(name=name, scene=scene, kind=kind, w=w, h=h, spp=spp, seed=seed, integrator=integ,
                                bounces=bounces))
    return out


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def load_scene(name):
    """The scene of LOADS[name] through the product's loader, BVH built."""
    import cudapathtracer_amd as pt
    s = pt.Scene()
    for obj, origin, scale, flip in LOADS[name]:
        s.load_obj(os.path.join(MODELS, obj), origin, scale, flip, mtl_basepath=MODELS + "/")
    s.build_bvh()
    return s


def morton(x, y):
    r = 0
    for b in range(16):
        r |= ((int(x) >> b) & 1) << (2 * b)
        r |= ((int(y) >> b) & 1) << (2 * b + 1)
    return r


def morton_grid(w, h):
    """Morton index of every pixel, scanline order."""
    return np.array([morton(x, y) for y in range(h) for x in range(w)], dtype=np.uint64)


# Where the caller rays of a scene start and point, when not anywhere in its bounding box: (centre, radius, axis,
# spread).  quirks is a handful of slivers up to 123456 units long: rays drawn in its bounding box leave integrator 1
# undefined on 87% of the samples, so its free rays start near the camera position above and point roughly along -z.
RAY_REGION = {"quirks": ((2.88, -0.78, 0.15), 1.0, (0.0, 0.0, -1.0), 0.4)}


def caller_rays(verts, n, rng, pad=0.1, region=None):
    """n regular rays for a scene with vertices verts (float32 (V, 3)): origins uniform in the bounding box grown by
    `pad` of its size (negative: shrunk, to stay inside a closed scene), or in the ball of `region`; every third origin
    EXACTLY a vertex (so bounces start with closestT < 0.001 and on edges shared by several triangles); unit
    directions, uniform or (region) scattered about an axis, every eighth along a coordinate axis (either sign)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    pad = pad * (hi - lo)
    o = rng.uniform(lo - pad, hi + pad, (n, 3))
    d = rng.normal(size=(n, 3))
    if region is not None:
        centre, radius, axis, spread = region
        o = np.asarray(centre) + radius * rng.uniform(-1, 1, (n, 3))
        d = np.asarray(axis) + spread * d
    o = o.astype(np.float32)
    on = np.arange(n) % 3 == 0
    pool = v if pad.min() >= 0 else v[np.all((v > lo) & (v < hi), axis=1)]   # closed scene: not its outer corners,
    o[on] = pool[rng.integers(0, len(pool), int(on.sum()))]                  # where a ray slips out between two walls
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = np.arange(n) % 8 == 1
    axes = np.zeros((int(ax.sum()), 3))
    axes[np.arange(len(axes)), rng.integers(0, 3, len(axes))] = rng.choice([-1.0, 1.0], len(axes))
    d[ax] = axes
    return np.concatenate([o, d.astype(np.float32)], axis=1)


def same_bits(a, b):
    """Elementwise: two float arrays of one dtype agree in every bit (signed zeros count), or are both NaN (the NaN
    PATTERN is compared; a NaN's sign and payload are the compiler's choice of instruction, not the integrator's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
