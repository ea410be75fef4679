"""Cases for the ray queries on device buffers (pt_trace_device, pt_occluded*): for a scene's arrays, the ray sets
and the tmax vectors, and the expected answers from the CPU oracle alone.

Ray sets come from raysets.py: ray_sets and bounce_rays (what the integrator makes, plus the slab test's edge cases;
"tiny" leaves the Markstein ranges and takes trace_slow), far_sets, range_edge_sets and regular_edge_sets (what only
a caller makes: rays that are not ray_fast take trace_slow, rays that are not ray_regular the reference's walk).

For a ray whose oracle hit is t*, the tmax classes and the answer of occ = (tri >= 0) & (t* < tmax) in float32:

    at        t*                   0  (strict)
    above     nextafter(t*, +inf)  1
    below     nextafter(t*, -inf)  0
    half      0.5 t*               0  (the ray has a hit, beyond tmax: an unbounded any-hit gets this one wrong)
    double    2 t*                 1
    inf       +inf                 1
    max       1e5                  1
    zero, negzero, minus_one       0
    nan                            0
    denormal  the smallest one     0

A miss (tri = -1, t = 1e5) gives 0 in every class."""
import numpy as np

from raysets import (COORD_HI, COORD_LO, DIR_HI, DIR_LO, DIR_LEN2_MAX, ORIGIN_EXTENTS, bounce_rays, far_sets,
                     range_edge_sets, ray_sets, regular_edge_sets)

F = np.float32
MAX_FLOAT = F(1e5)
TMAX_CLASSES = ("at", "above", "below", "half", "double", "inf", "max", "zero", "negzero", "minus_one", "nan", "denormal")
# classes in which a hit ray's answer is 1 (so that hits and misses give both answers); in the others every ray's is 0
CLASSES_WITH_BOTH = ("above", "double", "inf", "max")


def tmax_of_class(t, name):
    """The class's tmax for rays whose oracle distance is t (float32[n])."""
    t = np.asarray(t, dtype=F)
    const = {"inf": np.inf, "max": MAX_FLOAT, "zero": 0.0, "negzero": -0.0, "minus_one": -1.0, "nan": np.nan,
             "denormal": np.nextafter(F(0), F(1))}
    if name in const:
        return np.full(t.shape, const[name], dtype=F)
    if name == "at":
        return t.copy()
    if name == "above":
        return np.nextafter(t, F(np.inf))
    if name == "below":
        return np.nextafter(t, F(-np.inf))
    if name == "half":
        return (F(0.5) * t).astype(F)
    if name == "double":
        return (F(2.0) * t).astype(F)
    raise KeyError(name)


def tmax_cycle(t, offset=0):
    """(tmax float32[n], class index int[n]): ray i gets class (i + offset) mod 12."""
    t = np.asarray(t, dtype=F)
    cls = (np.arange(len(t)) + offset) % len(TMAX_CLASSES)
    tm = np.empty(len(t), dtype=F)
    for k, name in enumerate(TMAX_CLASSES):
        m = cls == k
        tm[m] = tmax_of_class(t[m], name)
    return tm, cls


def expected_occ(tri, t, tmax):
    """The definition, evaluated in float32 on the oracle's (tri, t): uint8[n].  tmax None: 1e5 for every ray."""
    t = np.asarray(t, dtype=F)
    tm = np.full(t.shape, MAX_FLOAT, dtype=F) if tmax is None else np.asarray(tmax, dtype=F)
    assert t.dtype == F and tm.dtype == F
    return ((np.asarray(tri) >= 0) & (t < tm)).astype(np.uint8)


def integrator_sets(arrays, n, seed, trace):
    """ray_sets plus the bounce rays of its interior set; trace(o, d) -> (tri, t) is the oracle's trace_batch."""
    sets = dict(ray_sets(arrays, n, seed))
    o, d = sets["interior"]
    tri, t = trace(o, d)
    sets["bounce"] = bounce_rays(arrays, o, d, tri, t, seed + 1)
    return sets


def fallback_sets(arrays, n, seed):
    """The sets that exist to reach the exact walks: origins to 2^20, direction scales 2^-101..2^100, both sides of
    the two ray_regular bounds."""
    sets = dict(far_sets(arrays, n, seed))
    sets.update(range_edge_sets(arrays, n, seed))
    sets.update(regular_edge_sets(arrays, n, seed))
    return sets


# ---------------------------------------------------------------- which walk a ray takes (pt_device.h), in numpy
def ray_fast(o, d):
    ao, ad = np.abs(o), np.abs(d)
    return (((ao == 0) | ((ao >= COORD_LO) & (ao <= COORD_HI))).all(axis=1) &
            ((ad == 0) | ((ad >= DIR_LO) & (ad <= DIR_HI))).all(axis=1))


def ray_regular(arrays, o, d):
    v = arrays["verts"]
    bound = F(ORIGIN_EXTENTS) * F(max(np.abs(v[k]).max() for k in "xyz"))
    with np.errstate(over="ignore"):
        len2 = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
    return (np.abs(o).max(axis=1) <= bound) & (len2 <= DIR_LEN2_MAX)


def walk_class(arrays, o, d):
    """0: the BVH4 walk (regular and fast), 1: trace_slow (regular, not fast), 2: the reference's walk."""
    reg = ray_regular(arrays, o, d)
    return np.where(~reg, 2, np.where(ray_fast(o, d), 0, 1))
