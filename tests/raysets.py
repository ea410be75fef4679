"""Ray sets for the ray-level parity tests and the trace() goldens (tools/make_golden.py).

What the integrator produces (camera rays, rays leaving surfaces at t - 0.001) plus the edge
cases of the slab test (axis-parallel rays, zero direction components, origins on box planes
and vertices, tiny components that leave the Markstein range, rays from outside the scene) -- ray_sets(), whose draws the goldens depend on.

far_sets(), range_edge_sets() and regular_edge_sets() hold rays only a caller of pt_trace makes: origins far from
the scene, components at the bounds of the fast walk's ranges, unnormalised directions
(tests/test_ray_ranges_host.py, tests/test_gpu_ray_ranges.py)."""
import numpy as np


def _unit(v):
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def ray_sets(arrays, n, seed):
    """Dict of named (origins, directions) float32 arrays over the scene's bounds."""
    rng = np.random.default_rng(seed)
    v = arrays["verts"]
    P = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = hi - lo
    out = {}
    o = rng.uniform(lo + 0.05 * ext, hi - 0.05 * ext, (n, 3))
    out["interior"] = (o.astype(np.float32), _unit(rng.normal(size=(n, 3))))
    d = rng.normal(size=(n, 3))
    axis = rng.integers(0, 3, n)
    zero = rng.integers(0, 3, n)
    d[np.arange(n), zero] = 0.0                     # one zero component
    d[: n // 3] = 0.0
    d[np.arange(n // 3), axis[: n // 3]] = rng.choice([-1.0, 1.0], n // 3)   # axis-parallel
    out["axis"] = (o.astype(np.float32), _unit(d))
    # origins on vertices and on their coordinate planes
    pick = P[rng.integers(0, len(P), n)]
    o2 = pick.copy()
    o2[n // 2:, 0] = rng.uniform(lo[0], hi[0], n - n // 2)
    out["vertex_planes"] = (o2.astype(np.float32), _unit(rng.normal(size=(n, 3))))
    # tiny components: outside the Markstein preconditions (exact slow path)
    d3 = rng.normal(size=(n, 3))
    d3[:, 1] = rng.choice([1e-31, -1e-36, 3e-39, 1e-20], n)
    out["tiny"] = (o.astype(np.float32), _unit(d3))
    # from outside: aimed at the scene
    c = 0.5 * (lo + hi)
    far = c + _unit(rng.normal(size=(n, 3))) * (2.0 * np.linalg.norm(ext) + 1.0)
    tgt = rng.uniform(lo, hi, (n, 3))
    out["outside"] = (far.astype(np.float32), _unit(tgt - far))
    return out


def _bounds(arrays):
    v = arrays["verts"]
    P = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64)
    return P, P.min(0), P.max(0)


# The fast walk's per-ray preconditions (pt_device.h coord_ok / dir_ok): a component is 0 or its magnitude lies
# in [COORD_LO, COORD_HI] (origins, scene coordinates) or [DIR_LO, DIR_HI] (directions).
COORD_LO, COORD_HI = np.float32(2.0 ** -50), np.float32(2.0 ** 20)
DIR_LO, DIR_HI = np.float32(2.0 ** -100), np.float32(2.0 ** 45)
FAR_DISTS = (1e3, 1e4, 5e4)
FAR_EDGE_DIST = 2.0 ** 20 - 4096.0      # with the scene centre added, every |o_k| stays below 2^20
DIR_SCALES = (-101, -100, -99, -60, -20, 20, 44, 45, 46, 60, 100)


def neighbours(b):
    """(the float below b, b, the float above b) in magnitude, as float32."""
    b = np.float32(b)
    return np.nextafter(b, np.float32(0.0)), b, np.nextafter(b, np.float32(np.inf))


def far_sets(arrays, n, seed):
    """Rays from far outside, aimed at uniform points of the scene's bounds: origins on spheres about the scene
    centre at FAR_DISTS with unit directions, and one rung just below the origin bound 2^20 with |d| = 2^10
    (so that t = distance / |d| stays below MAX_FLOAT = 1e5)."""
    rng = np.random.default_rng(seed)
    _, lo, hi = _bounds(arrays)
    c = 0.5 * (lo + hi)
    out = {}
    for name, dist, scale in [("far_%g" % x, x, 1.0) for x in FAR_DISTS] + [("far_2p20_d1024", FAR_EDGE_DIST, 1024.0)]:
        o = (c + _unit(rng.normal(size=(n, 3))).astype(np.float64) * dist).astype(np.float32)
        tgt = rng.uniform(lo, hi, (n, 3))
        out[name] = (o, _unit(tgt - o.astype(np.float64)) * np.float32(scale))
    return out


def _orders(n, classes):
    """Class of ray i in the two orders: interleaved ray by ray (every wave of 64 mixes the classes) and in
    runs of 64 (whole waves of one class)."""
    i = np.arange(n)
    return {"mixed": i % classes, "runs": (i // 64) % classes}


def range_edge_sets(arrays, n, seed):
    """Rays at the bounds of the fast walk's preconditions, over a hit-rich base (interior origins; directions
    half aimed at vertices, half random).  Three families, each in the two orders of _orders():
      dir_scale    the whole direction times 2^k, k in DIR_SCALES
      dir_comp     one direction component set to +-b for b in the four bounds and the floats next to them
      origin_comp  one origin coordinate set to +-b for the coordinate bounds and their neighbours, to -0.0,
                   a denormal (1e-40), 3e6 and 1e30; origins moved far out get a direction aimed back at the
                   scene with |d| = 2^10
    No zero direction vector and no non-finite component."""
    rng = np.random.default_rng(seed)
    P, lo, hi = _bounds(arrays)
    ext = hi - lo
    o = rng.uniform(lo + 0.05 * ext, hi - 0.05 * ext, (n, 3))
    d = rng.normal(size=(n, 3))
    d[: n // 2] = P[rng.integers(0, len(P), n // 2)] - o[: n // 2]
    perm = rng.permutation(n)            # aimed and random rays in every class
    o, d = o[perm].astype(np.float32), _unit(d[perm])
    comp = rng.integers(0, 3, n)
    sign = rng.choice(np.float32([-1.0, 1.0]), n)
    tgt = rng.uniform(lo, hi, (n, 3))
    rows = np.arange(n)
    dvals = np.float32([v for b in (DIR_LO, DIR_HI, COORD_LO, COORD_HI) for v in neighbours(b)])
    ovals = np.float32([v for b in (COORD_LO, COORD_HI) for v in neighbours(b)] + [1e-40, 3e6, 1e30])
    out = {}
    for order, cls in _orders(n, len(DIR_SCALES)).items():
        k = np.array(DIR_SCALES, dtype=np.float64)[cls]
        out["dir_scale_" + order] = (o.copy(), (d.astype(np.float64) * (2.0 ** k)[:, None]).astype(np.float32))
    for order, cls in _orders(n, len(dvals)).items():
        d2 = d.copy()
        d2[rows, comp] = sign * dvals[cls]
        out["dir_comp_" + order] = (o.copy(), d2)
    for order, cls in _orders(n, len(ovals) + 1).items():
        o2, d2 = o.copy(), d.copy()
        val = np.where(cls < len(ovals), sign * ovals[np.minimum(cls, len(ovals) - 1)], np.float32(-0.0))
        o2[rows, comp] = val.astype(np.float32)
        moved = np.abs(val) >= 1.0       # (2^20 and its neighbours, 3e6, 1e30: far outside the scene)
        aim = _unit(tgt - o2.astype(np.float64)) * np.float32(1024.0)
        d2[moved] = aim[moved]
        out["origin_comp_" + order] = (o2, d2)
    return out


ORIGIN_EXTENTS = 64.0                   # pt_device.h ray_regular: |o_k| <= 64 scene extents ...
DIR_LEN2_MAX = np.float32(1.0 + 2.0 ** -10)   # ... and |d|^2 <= 1 + 2^-10, else the reference's own walk


def regular_edge_sets(arrays, n, seed):
    """Rays on both sides of the two bounds beyond which pt_trace leaves the culled walks (ray_regular), classes
    interleaved ray by ray: "origin_bound" has one origin coordinate at +-64 extents, the float below and the
    float above (unit directions aimed at the scene); "dir_length" scales unit directions from interior origins
    by 1, 1.0004 (|d|^2 just below 1 + 2^-10), 1.0006 (just above) and 2."""
    rng = np.random.default_rng(seed)
    P, lo, hi = _bounds(arrays)
    ext = hi - lo
    bound = np.float32(ORIGIN_EXTENTS) * np.float32(np.abs(P).max())
    rows = np.arange(n)
    o = rng.uniform(lo, hi, (n, 3))
    comp = rng.integers(0, 3, n)
    vals = np.float32(neighbours(bound))[rows % 3] * rng.choice(np.float32([-1.0, 1.0]), n)
    o[rows, comp] = vals
    o = o.astype(np.float32)
    out = {"origin_bound": (o, _unit(rng.uniform(lo, hi, (n, 3)) - o.astype(np.float64)))}
    o = rng.uniform(lo + 0.05 * ext, hi - 0.05 * ext, (n, 3)).astype(np.float32)
    scale = np.float32([1.0, 1.0004, 1.0006, 2.0])[rows % 4]
    out["dir_length"] = (o, _unit(rng.normal(size=(n, 3))) * scale[:, None])
    return out


def bounce_rays(arrays, o, d, tri, t, seed):
    """Rays leaving the surfaces hit by (o, d) the way the integrator builds them
    (kernel.cu:455-470: pos = o + d * (float)(t - 0.001))."""
    rng = np.random.default_rng(seed)
    hit = tri >= 0
    tt = (t[hit].astype(np.float64) - 0.001).astype(np.float32)
    pos = (o[hit] + d[hit] * tt[:, None]).astype(np.float32)
    return pos, _unit(rng.normal(size=(len(pos), 3)))
