"""Scenes as a caller builds them: plain arrays and a BVH made in numpy, handed to pt_create as a pt_scene.

Every other scene of the suite comes out of pt_scene_load_obj + pt_scene_build_bvh, one family of trees: breadth-first
node order, tight boxes, bvh_depth equal to the true depth, at most 25 levels.  The builders here keep a loaded
fixture's triangles, vertices and materials and replace the reference BVH (and, in caller_data, the lists the loader
writes in one fixed way).  Each returns arrays that meet the contract of pt.h (pt_scene): a tree over the triangles,
finite boxes, every child box within its parent's, every triangle within its parent node's box, true depth <=
bvh_depth < 64.  check_contract() restates that in numpy; tests/test_caller_scenes_host.py asserts it for every
builder, so a GPU test never sees an invalid tree.

The CPU oracle walks whatever BVH it is given (oracle.OracleScene(arrays)), so it is the reference for all of them.
"""
import ctypes as C
import os

import numpy as np

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
from cudapathtracer_amd.api import MAT, NODE, SPHERE, TRI, VEC3

LEAF = 0x80000000
F = np.float32
BIG = F(1572864.0)          # 1.5 * 2^20: a box coordinate beyond the Markstein range of scene coordinates (2^20)
WIDE = F(524288.0)          # 2^19: a root box far larger than the geometry, still inside that range
BUILDER_NAMES = ("library", "swapped", "median", "permuted", "median_permuted", "loose", "loose_big", "loose_root",
                 "overstated7", "overstated63", "caller_data")
CHAIN_NAMES = ("chain_left", "chain_right", "chain_left_permuted")


class ArrayScene:
    """A scene held as numpy arrays; view() is the pt_scene over them (pt.Renderer(scene, 0) needs nothing more)."""

    def __init__(self, arrays, bvh_depth=None):
        a = dict(arrays)
        self._a = dict(
            verts=np.ascontiguousarray(a["verts"], dtype=VEC3), tris=np.ascontiguousarray(a["tris"], dtype=TRI),
            mats=np.ascontiguousarray(a["mats"], dtype=MAT), lights=np.ascontiguousarray(a["lights"], dtype=np.uint32),
            total_light_area=F(a["total_light_area"]), bvh=np.ascontiguousarray(a["bvh"], dtype=NODE),
            bvh_depth=int(a["bvh_depth"] if bvh_depth is None else bvh_depth),
            spheres=np.ascontiguousarray(a.get("spheres", np.zeros(0, dtype=SPHERE)), dtype=SPHERE))

    def arrays(self):
        return dict(self._a)

    def view(self):
        a = self._a
        v = _lib.SceneView()

        def ptr(arr, ctype):
            return arr.ctypes.data_as(C.POINTER(ctype)) if len(arr) else None
        v.num_verts, v.num_tris, v.num_mats, v.num_lights = len(a["verts"]), len(a["tris"]), len(a["mats"]), len(a["lights"])
        v.verts, v.tris, v.mats = ptr(a["verts"], _lib.Vec3), ptr(a["tris"], _lib.Triangle), ptr(a["mats"], _lib.Material)
        v.lights = ptr(a["lights"], C.c_uint32)
        v.total_light_area = float(a["total_light_area"])
        v.bvh, v.bvh_size, v.bvh_depth = ptr(a["bvh"], _lib.BvhNode), len(a["bvh"]), a["bvh_depth"]
        v.spheres, v.num_spheres = ptr(a["spheres"], _lib.Sphere), len(a["spheres"])
        return v

    def create(self):
        """(handle, error code, message) of pt_create on device 0; the caller destroys a non-null handle."""
        v = self.view()
        err = C.c_int(0)
        h = _lib.lib().pt_create(C.byref(v), 0, C.byref(err))
        return h, err.value, (_lib.lib().pt_last_error() or b"").decode(errors="replace")

    def accel_digest(self):
        v = self.view()
        dg, n4, d4 = C.c_uint64(), C.c_uint32(), C.c_int32()
        _lib.check(_lib.lib().pt_accel_digest(C.byref(v), C.byref(dg), C.byref(n4), C.byref(d4)))
        return int(dg.value), int(n4.value), int(d4.value)


# ---------------------------------------------------------------- the contract, in numpy
def tri_points(a):
    """(nt, 3, 3) float32: the vertices of every triangle."""
    v = a["verts"]
    V = np.stack([v["x"], v["y"], v["z"]], axis=1)
    t = a["tris"]
    return V[np.stack([t["v0"], t["v1"], t["v2"]], axis=1)]


def true_depth(bvh):
    """A leaf counts 1, a node 1 + its deeper child (BVH_node::depth)."""
    deepest, st = 0, [(0, 1)]
    while st:
        e, level = st.pop()
        for c in (int(bvh["left"][e]), int(bvh["right"][e])):
            if c & LEAF:
                deepest = max(deepest, level + 1)
            else:
                st.append((c, level + 1))
    return deepest


def check_contract(a):
    """The violations of pt.h's pt_scene contract, as a list of strings (empty: valid)."""
    b, nt = a["bvh"], len(a["tris"])
    bad = []
    if len(b) != nt - 1:
        return ["%d nodes for %d triangles" % (len(b), nt)]
    if not (np.isfinite(b["lo"]).all() and np.isfinite(b["hi"]).all()):
        bad.append("box coordinate not finite")
    P = tri_points(a)
    seen_t, seen_n = np.zeros(nt, int), np.zeros(len(b), int)
    seen_n[0] = 1
    st = [0]
    while st:
        e = st.pop()
        for c in (int(b["left"][e]), int(b["right"][e])):
            if c & LEAF:
                k = c ^ LEAF
                if k >= nt:
                    return bad + ["leaf %d out of range" % k]
                seen_t[k] += 1
                if not ((P[k] >= b["lo"][e]).all() and (P[k] <= b["hi"][e]).all()):
                    bad.append("triangle %d outside node %d" % (k, e))
            else:
                if c >= len(b):
                    return bad + ["child %d out of range" % c]
                seen_n[c] += 1
                if seen_n[c] > 1:
                    return bad + ["node %d reached twice" % c]
                if not ((b["lo"][c] >= b["lo"][e]).all() and (b["hi"][c] <= b["hi"][e]).all()):
                    bad.append("node %d outside node %d" % (c, e))
                st.append(c)
    if not ((seen_t == 1).all() and (seen_n == 1).all()):
        bad.append("not every triangle and node reached once")
    d = true_depth(b)
    if not d <= a["bvh_depth"] < 64:
        bad.append("true depth %d, bvh_depth %d" % (d, a["bvh_depth"]))
    return bad


# ---------------------------------------------------------------- BVH builders
def _with_bvh(a, bvh, depth=None):
    out = dict(a)
    out["bvh"] = bvh
    out["bvh_depth"] = true_depth(bvh) if depth is None else depth
    return out


def swapped(a):
    """Left and right exchanged at every node: the DFS order reverses, so the other copy of a duplicate wins."""
    b = a["bvh"].copy()
    b["left"], b["right"] = a["bvh"]["right"].copy(), a["bvh"]["left"].copy()
    return _with_bvh(a, b)


def median(a):
    """Top-down median split on the longest centroid axis, ties in input order; tight boxes (exact float32 min / max
    of the vertices); nodes numbered depth-first, so neither the leaves nor the nodes come in the library's order."""
    P = tri_points(a)
    cen = P.astype(np.float64).mean(axis=1)
    nodes = np.zeros(len(P) - 1, dtype=NODE)
    used = [0]

    def build(ids):
        if len(ids) == 1:
            return LEAF | int(ids[0])
        i = used[0]
        used[0] += 1
        nodes["lo"][i] = P[ids].reshape(-1, 3).min(axis=0)
        nodes["hi"][i] = P[ids].reshape(-1, 3).max(axis=0)
        ext = cen[ids].max(axis=0) - cen[ids].min(axis=0)
        order = ids[np.argsort(cen[ids, int(np.argmax(ext))], kind="stable")]
        half = len(order) // 2
        nodes["left"][i] = build(order[:half])
        nodes["right"][i] = build(order[half:])
        return i

    build(np.arange(len(P)))
    assert used[0] == len(nodes)
    return _with_bvh(a, nodes)


def permuted(a, seed):
    """The node array shuffled (the root stays node 0): children may have smaller indices than their parents."""
    b = a["bvh"]
    rng = np.random.default_rng(seed)
    new_of = np.concatenate([[0], 1 + rng.permutation(len(b) - 1)]).astype(np.uint32)
    out = np.zeros_like(b)

    def remap(c):
        return np.where(c & LEAF != 0, c, new_of[np.minimum(c & ~np.uint32(LEAF), len(b) - 1)]).astype(np.uint32)
    out[new_of] = b
    out["left"], out["right"] = remap(out["left"]), remap(out["right"])
    return _with_bvh(a, out, a["bvh_depth"])


def loose(a, seed, big=None):
    """The boxes grown outwards, top-down, a child never beyond its parent, so nesting holds: each node by 1 ulp, 1e-3
    or 0.5 (its own draw per node).  big: the root and the nodes down one path also get hi.x = big: BIG, so that the
    boxes, not the vertices, leave the Markstein range, or WIDE, a root box 2^19 wide around geometry a few units
    across (the scene's extent, which bounds the origins the culled walks take, must stay the geometry's)."""
    b = a["bvh"].copy()
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, len(b))
    path = set()
    if big is not None:
        e = 0
        for _ in range(4):
            path.add(e)
            c = int(b["left"][e]) if not int(b["left"][e]) & LEAF else int(b["right"][e])
            if c & LEAF:
                break
            e = c
    st = [(0, None)]
    while st:
        e, p = st.pop()
        lo, hi = b["lo"][e].copy(), b["hi"][e].copy()
        if kind[e] == 0:
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        else:
            g = F(1e-3) if kind[e] == 1 else F(0.5)
            lo, hi = lo - g, hi + g
        if big != BIG:
            # one ulp below a coordinate that is 0 is a denormal, which (rightly) takes the whole scene off the
            # Markstein quotient; loose_big keeps those, the others step to -+2^-50, the smallest magnitude in range
            tiny = F(2.0 ** -50)
            lo = np.where((lo != 0) & (np.abs(lo) < tiny), -tiny, lo)
            hi = np.where((hi != 0) & (np.abs(hi) < tiny), tiny, hi)
        if e in path:
            hi[0] = big
        if p is not None:
            lo, hi = np.maximum(lo, b["lo"][p]), np.minimum(hi, b["hi"][p])
        b["lo"][e], b["hi"][e] = lo, hi
        for c in (int(b["left"][e]), int(b["right"][e])):
            if not c & LEAF:
                st.append((c, e))
    return _with_bvh(a, b, a["bvh_depth"])


def chain(a, lean):
    """A chain over all k triangles of `a`, true depth k: node i holds triangle i and the chain of the triangles after
    it, which is its left child (lean = "left": visited first, the stack grows to the full depth) or its right."""
    P = tri_points(a)
    k = len(P)
    nodes = np.zeros(k - 1, dtype=NODE)
    for i in range(k - 1):
        nodes["lo"][i] = P[i:].reshape(-1, 3).min(axis=0)
        nodes["hi"][i] = P[i:].reshape(-1, 3).max(axis=0)
        rest = (i + 1) if i < k - 2 else (LEAF | (k - 1))
        nodes["left"][i], nodes["right"][i] = (rest, LEAF | i) if lean == "left" else (LEAF | i, rest)
    out = _with_bvh(a, nodes)
    assert out["bvh_depth"] == k
    return out


def overstated(a, depth):
    """bvh_depth larger than the true depth: must behave exactly as the honest value."""
    assert depth > true_depth(a["bvh"])
    return _with_bvh(a, a["bvh"], depth)


# ---------------------------------------------------------------- scene data the loader never produces
def light_areas(a):
    """The area of every light-list entry, float32, by the integrator's formulas (kernel.cu:477-478; spheres
    4 * 3.14159 * r^2)."""
    P = tri_points(a)
    out = np.zeros(len(a["lights"]), dtype=F)
    for j, e in enumerate(a["lights"]):
        e = int(e)
        if e & _lib.PT_LIGHT_SPHERE:
            r = F(a["spheres"]["rad"][e ^ _lib.PT_LIGHT_SPHERE])
            out[j] = F(F(F(4.0) * F(3.14159)) * r) * r
        else:
            e1, e2 = P[e, 1] - P[e, 0], P[e, 2] - P[e, 0]
            c = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=F)
            out[j] = np.sqrt(F(F(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])) / F(2)
    return out


def caller_data(a, seed):
    """The same geometry with the lists written another way: equal vertices merged (triangles share indices, the
    merged-away vertices stay in the array unused), `norm` flipped on a tenth of the triangles and scaled by 2 or 0.5
    on another fifth, the light list reversed with sphere entries moved between the triangle entries, and
    total_light_area summed in that order."""
    rng = np.random.default_rng(seed)
    out = dict(a)
    v = a["verts"]
    V = np.stack([v["x"], v["y"], v["z"]], axis=1)
    _, first = np.unique(V.view(np.uint32), axis=0, return_index=True)
    _, inverse = np.unique(V.view(np.uint32), axis=0, return_inverse=True)
    canon = first[inverse.reshape(-1)]
    t = a["tris"].copy()
    for f in ("v0", "v1", "v2"):
        t[f] = canon[t[f]]
    u = rng.random(len(t))
    s = np.where(u < 0.1, -1.0, np.where(u < 0.2, 2.0, np.where(u < 0.3, 0.5, 1.0))).astype(F)
    for f in ("nx", "ny", "nz"):
        t[f] = t[f] * s
    out["tris"] = t
    li = a["lights"][::-1].copy()
    sph = [e for e in li if int(e) & _lib.PT_LIGHT_SPHERE]
    tri = [e for e in li if not int(e) & _lib.PT_LIGHT_SPHERE]
    mixed = []
    while sph or tri:
        if tri:
            mixed.append(tri.pop(0))
        if sph:
            mixed.append(sph.pop(0))
    out["lights"] = np.array(mixed, dtype=np.uint32)
    total = F(0)
    for x in light_areas(out):
        total = F(total + x)
    out["total_light_area"] = total
    return out


def glowing(a):
    """Every dark material given emission 0.5 * albedo (the light list stays the caller's): each primary hit shows
    its material, so that which copy of a duplicate wins is visible in the image."""
    out = dict(a)
    m = a["mats"].copy()
    dark = m["emission"][:, 0] == 0
    m["emission"][dark] = 0.5 * m["albedo"][dark]
    out["mats"] = m
    return out


# ---------------------------------------------------------------- base scenes
def load_soup(dirpath, seed=11):
    from test_gpu_random_scenes import write_soup
    p = write_soup(dirpath, seed)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    return s.arrays()


def load_cornell(spheres=False):
    from conftest import load_scene
    import light_scenes as ls
    s = load_scene("cornell", build_bvh=False)
    if spheres:
        ls.add_random_spheres(s, 7, 6, 2, box=((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0)))
    s.build_bvh()
    return s.arrays()


def soup_subset(soup, k=63):
    """k triangles of the soup, for the chains: k - 22 random ones, the 20 duplicates (14 of them of triangles kept
    when k = 63: exact ties) and the light quad.  The vertex array stays whole, so most of it is unused."""
    nt = len(soup["tris"])
    keep = np.array(list(range(k - 22)) + list(range(220, 240)) + [nt - 2, nt - 1])
    assert len(keep) == k
    new_of = np.full(nt, -1)
    new_of[keep] = np.arange(len(keep))
    out = dict(soup)
    out["tris"] = soup["tris"][keep].copy()
    out["lights"] = new_of[soup["lights"]].astype(np.uint32)
    assert (new_of[soup["lights"]] >= 0).all()
    out["bvh"], out["bvh_depth"] = None, 0
    return out


def builders(base, chains=False):
    """name -> arrays: every builder on one base scene (chains: the base is the 63-triangle subset)."""
    if chains:
        left, right = chain(base, "left"), chain(base, "right")
        out = {"chain_left": left, "chain_right": right, "chain_left_permuted": permuted(left, 5)}
        assert tuple(out) == CHAIN_NAMES
        return out
    out = {"library": base, "swapped": swapped(base), "median": median(base)}
    out["permuted"] = permuted(base, 1)
    out["median_permuted"] = permuted(out["median"], 2)
    out["loose"] = loose(out["swapped"], 3)
    out["loose_big"] = loose(base, 4, big=BIG)
    out["loose_root"] = loose(out["median"], 7, big=WIDE)
    d = true_depth(base["bvh"])
    out["overstated7"] = overstated(out["median"], true_depth(out["median"]["bvh"]) + 7)
    out["overstated63"] = overstated(base, 63)
    assert d == base["bvh_depth"]
    out["caller_data"] = caller_data(out["median_permuted"], 6)
    assert tuple(sorted(out)) == tuple(sorted(BUILDER_NAMES))
    return out


def geometry_extent(a):
    """The largest coordinate magnitude of the vertices the triangles use and of the spheres (float32)."""
    ext = np.abs(tri_points(a)).max()
    for s in a.get("spheres", ()):
        ext = max(ext, (np.abs(s["pos"]) + s["rad"]).max())
    return F(ext)


# ---------------------------------------------------------------- rays
def _unit(v):
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)


def surface_points(a, n, rng):
    """n points on triangles picked by area-blind index (float64)."""
    P = tri_points(a).astype(np.float64)
    k = rng.integers(0, len(P), n)
    u = rng.random((n, 2))
    flip = u.sum(axis=1) > 1
    u[flip] = 1 - u[flip]
    return P[k, 0] + (P[k, 1] - P[k, 0]) * u[:, :1] + (P[k, 2] - P[k, 0]) * u[:, 1:]


def ray_sets(a, n, seed, trace):
    """Named (origins, directions): raysets.py's interior and tiny sets and the bounce rays of the former; interior
    origins aimed at vertices; "zero": one or two zero direction components, aimed at surface points (the ancestor
    walk of the winner check); "far": origins 1000 units out, beyond ray_regular's 64 extents, aimed at surface points
    (the reference's own walk, its stack in the lane's memory column).  trace(o, d) is the oracle's."""
    import raysets
    rng = np.random.default_rng(seed)
    t_ = a["tris"]
    used = np.unique(np.concatenate([t_["v0"], t_["v1"], t_["v2"]]))
    base = raysets.ray_sets(dict(a, verts=a["verts"][used]), n, seed)   # (bounds of the vertices in use)
    out = {}
    for name in ("interior", "tiny"):   # the second half moved along its direction to pass through a surface point
        o, d = base[name]
        o = o.copy()
        h = n // 2
        o[h:] = (surface_points(a, n - h, rng) - d[h:].astype(np.float64) * rng.uniform(0.1, 2.0, (n - h, 1))).astype(F)
        out[name] = (o, d)
    o, d = out["interior"]
    tri, t = trace(o, d)
    out["bounce"] = raysets.bounce_rays(a, o, d, tri, t, seed + 1)
    P = tri_points(a).reshape(-1, 3).astype(np.float64)
    tgt = P[rng.integers(0, len(P), n)]
    dv = tgt - o.astype(np.float64)
    dv[np.linalg.norm(dv, axis=1) == 0] = (0.0, -1.0, 0.0)
    out["vertices"] = (o, _unit(dv))
    dz = rng.normal(size=(n, 3))
    k1 = rng.integers(0, 3, n)
    dz[np.arange(n), k1] = 0.0
    two = rng.random(n) < 0.3
    dz[two, (k1[two] + 1) % 3] = 0.0
    dz = _unit(dz)
    p = surface_points(a, n, rng)
    out["zero"] = ((p - dz.astype(np.float64) * rng.uniform(0.1, 2.0, (n, 1))).astype(F), dz)
    df = _unit(rng.normal(size=(n, 3)))
    out["far"] = ((surface_points(a, n, rng) - df.astype(np.float64) * 1000.0).astype(F), df)
    return out
