"""Caller-built scenes without a GPU: the builders of caller_scenes.py meet the pt_scene contract, the oracle walks
their trees and tells them apart, and pt_create refuses every BVH the device walks cannot take -- before it looks
for a device, so the refusals below are the same with and without one."""
import ctypes as C
import os

import numpy as np
import pytest

from cudapathtracer_amd import _lib

import caller_scenes as cs

F = np.float32


@pytest.fixture(scope="module")
def bases(tmp_path_factory):
    soup = cs.load_soup(str(tmp_path_factory.mktemp("caller_soup")))
    return {"cornell": cs.load_cornell(), "soup": soup, "cornell_spheres": cs.load_cornell(True)}


@pytest.fixture(scope="module")
def built(bases):
    """(base, builder) -> arrays, every builder on every base and the chains on the 63-triangle subset."""
    out = {}
    for name in ("cornell", "soup", "cornell_spheres"):
        for k, a in cs.builders(bases[name]).items():
            out[name, k] = a
    for k, a in cs.builders(cs.soup_subset(bases["soup"]), chains=True).items():
        out["subset", k] = a
    return out


def _refused(arrays, code, *words):
    """pt_create refuses with `code` and a message holding every word; never a context."""
    h, rc, msg = cs.ArrayScene(arrays).create()
    if h:
        _lib.lib().pt_destroy(h)
    assert not h and rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    return msg


def _parents(b):
    """(parent node of every node (root: -1), parent node of every triangle)."""
    pn, pt_ = np.full(len(b), -1), np.full(len(b) + 1, -1)
    for e in range(len(b)):
        for c in (int(b["left"][e]), int(b["right"][e])):
            if c & cs.LEAF:
                pt_[c ^ cs.LEAF] = e
            else:
                pn[c] = e
    return pn, pt_


# ---------------------------------------------------------------- the builders
def test_every_builder_meets_the_contract(built):
    assert len(built) == 3 * len(cs.BUILDER_NAMES) + len(cs.CHAIN_NAMES)
    for key, a in built.items():
        assert cs.check_contract(a) == [], key
        assert len(a["bvh"]) == len(a["tris"]) - 1


def test_builders_are_what_they_say(bases, built):
    soup = bases["soup"]
    assert len(soup["tris"]) == 310 and len(bases["cornell"]["tris"]) == 32
    b = built["soup", "permuted"]["bvh"]
    kids = np.concatenate([b["left"], b["right"]])
    inner = (kids & cs.LEAF) == 0
    parent_idx = np.concatenate([np.arange(len(b)), np.arange(len(b))])
    assert np.count_nonzero(kids[inner] < parent_idx[inner]) > 50          # children before their parents
    lb = soup["bvh"]
    lkids = np.concatenate([lb["left"], lb["right"]])
    assert (lkids[(lkids & cs.LEAF) == 0] > parent_idx[(lkids & cs.LEAF) == 0]).all()   # the library: breadth-first
    for name in ("chain_left", "chain_right", "chain_left_permuted"):
        a = built["subset", name]
        assert len(a["tris"]) == 63 and cs.true_depth(a["bvh"]) == 63 == a["bvh_depth"]
    assert built["soup", "overstated63"]["bvh_depth"] == 63 > cs.true_depth(soup["bvh"]) == soup["bvh_depth"]
    m = built["soup", "overstated7"]
    assert m["bvh_depth"] == cs.true_depth(m["bvh"]) + 7
    lo = built["soup", "loose"]
    grown = (lo["bvh"]["hi"] - built["soup", "swapped"]["bvh"]["hi"]).max(axis=1)
    assert (grown > 0.4).any() and ((grown > 0) & (grown < 1e-5)).any() and ((grown > 5e-4) & (grown < 2e-3)).any()
    assert np.abs(np.stack([lo["verts"][k] for k in "xyz"])).max() < 2.0 ** 20
    assert np.abs(lo["bvh"]["hi"]).max() < 2.0 ** 20
    for base in ("cornell", "soup", "cornell_spheres"):      # every box coordinate 0 or in [2^-50, 2^20]: the fast walk
        for k in ("loose", "loose_root"):
            m = np.abs(np.concatenate([built[base, k]["bvh"]["lo"], built[base, k]["bvh"]["hi"]]))
            assert ((m == 0) | ((m >= F(2.0 ** -50)) & (m <= F(2.0 ** 20)))).all(), (base, k)
    m = np.abs(built["cornell", "loose_big"]["bvh"]["lo"])
    assert ((m != 0) & (m < F(2.0 ** -50))).any()           # ... and here also a denormal, 1 ulp below a 0
    big = built["soup", "loose_big"]["bvh"]["hi"][:, 0]
    assert 2 <= np.count_nonzero(big > 2.0 ** 20) <= 4 and big[0] > 2.0 ** 20
    wide = built["soup", "loose_root"]["bvh"]["hi"]          # a root box 2^19 wide, inside the Markstein range
    assert wide[0, 0] == cs.WIDE and np.abs(wide).max() == cs.WIDE and np.abs(built["soup", "loose_root"]["bvh"]["lo"]).max() < 8
    assert cs.geometry_extent(built["soup", "loose_root"]) == cs.geometry_extent(soup) < 8
    cd, mp = built["soup", "caller_data"], built["soup", "median_permuted"]
    t = cd["tris"]
    idx = np.concatenate([t["v0"], t["v1"], t["v2"]])
    assert len(np.unique(idx)) < len(idx) and len(np.unique(idx)) < len(cd["verts"])      # shared and unused vertices
    assert np.array_equal(cs.tri_points(cd), cs.tri_points(mp))                            # the same geometry
    n2 = t["nx"].astype(np.float64) ** 2 + t["ny"].astype(np.float64) ** 2 + t["nz"].astype(np.float64) ** 2
    assert (n2 > 3).any() and ((n2 > 0.2) & (n2 < 0.3)).any()                              # not of unit length
    assert np.count_nonzero(np.signbit(t["nx"]) != np.signbit(mp["tris"]["nx"])) > 5        # flipped
    cds = built["cornell_spheres", "caller_data"]
    is_sph = (cds["lights"] & _lib.PT_LIGHT_SPHERE) != 0
    assert is_sph.any() and not is_sph.all() and (np.diff(is_sph.astype(int)) != 0).sum() >= 3   # interleaved
    assert sorted(cds["lights"]) == sorted(bases["cornell_spheres"]["lights"])
    ref = float(bases["cornell_spheres"]["total_light_area"])
    assert abs(float(cds["total_light_area"]) - ref) <= 4 * np.spacing(F(ref))


def test_the_oracle_and_pt_accel_digest_accept_every_builder(built):
    import oracle
    rng = np.random.default_rng(1)
    o = rng.uniform(-2, 2, (256, 3)).astype(F)
    d = cs._unit(rng.normal(size=(256, 3)))
    for key, a in built.items():
        tri, t = oracle.trace_batch(oracle.OracleScene(a), o, d)         # (raises at the oracle's 64-entry stack)
        assert ((tri >= -1) & (tri < len(a["tris"]) + len(a["spheres"]))).all(), key
        dg, n4, d4 = cs.ArrayScene(a).accel_digest()
        assert n4 > 0 and d4 > 0, key
    # the BVH4 is built from the triangles alone: the caller's tree does not change it
    for base in ("cornell", "soup"):
        assert len({cs.ArrayScene(built[base, k]).accel_digest() for k in ("library", "swapped", "median", "loose_big")}) == 1


def test_pt_create_validates_every_builder_before_the_device(built):
    """A valid scene gets past the validation: a context on a machine with a GPU, PT_E_NODEV on one without."""
    for key, a in built.items():
        h, rc, msg = cs.ArrayScene(a).create()
        if h:
            _lib.lib().pt_destroy(h)
        assert (h and rc == _lib.PT_OK) or (not h and rc == _lib.PT_E_NODEV), (key, rc, msg)


def test_the_library_s_own_trees_pass_unchanged(tmp_path, standin_scene):
    """pt_scene_build_bvh's output meets the contract on every fixture, the random soups and the 262K-triangle
    stand-in: pt_create gets past the validation (a context, or PT_E_NODEV without a GPU)."""
    import cudapathtracer_amd as pt
    from cudapathtracer_amd import scenes
    from conftest import load_scene
    import light_scenes as ls
    from test_gpu_random_scenes import write_soup

    def loaded(path):
        s = pt.Scene()
        s.load_obj(path, mtl_basepath=os.path.dirname(path) + "/")
        return s.build_bvh()
    made = {n: load_scene(n) for n in ("cornell", "cornell_blob", "quirks", "blob_flip", "quad")}
    made["splinters"] = loaded(scenes.write_splinters(str(tmp_path)))
    made["soup11"] = loaded(write_soup(str(tmp_path / "s11"), 11))
    made["soup14"] = loaded(write_soup(str(tmp_path / "s14"), 14))
    made["lit"] = loaded(ls.write_lit_soup(str(tmp_path / "lit"), 5, 7))
    made["standin"] = standin_scene
    for name, s in made.items():
        a = s.arrays()
        if name != "standin":      # (the numpy restatement is a Python loop: not on 262K triangles)
            assert cs.check_contract(a) == [], name
        assert cs.true_depth(a["bvh"]) == a["bvh_depth"], name
        v = s.view()
        err = C.c_int(0)
        h = _lib.lib().pt_create(C.byref(v), 0, C.byref(err))
        if h:
            _lib.lib().pt_destroy(h)
        assert err.value in (_lib.PT_OK, _lib.PT_E_NODEV), (name, err.value, _lib.lib().pt_last_error())


def test_the_oracle_tells_the_trees_apart(bases, built):
    """On the soup, exchanging the children changes the winner among exact duplicates (>= 1% of random rays) and no
    distance; looser boxes and another valid tree with the same tie order change nothing."""
    import oracle
    rng = np.random.default_rng(3)
    n = 20000
    o = rng.uniform(-2.5, 2.5, (n, 3)).astype(F)
    d = cs._unit(rng.normal(size=(n, 3)))
    tri0, t0 = oracle.trace_batch(oracle.OracleScene(bases["soup"]), o, d)
    res = {k: oracle.trace_batch(oracle.OracleScene(built["soup", k]), o, d) for k in
           ("swapped", "median", "loose", "loose_big", "loose_root", "permuted", "overstated63")}
    changed = int(np.count_nonzero(res["swapped"][0] != tri0))
    print("swapped: winners changed on %d of %d rays" % (changed, n))
    assert changed >= n // 100
    assert res["swapped"][1].tobytes() == t0.tobytes()
    assert res["loose"][0].tobytes() == res["swapped"][0].tobytes() and res["loose"][1].tobytes() == t0.tobytes()
    for k in ("median", "loose_big", "loose_root", "permuted", "overstated63"):
        assert res[k][0].tobytes() == tri0.tobytes() and res[k][1].tobytes() == t0.tobytes(), k


# ---------------------------------------------------------------- what pt_create refuses
def _mutable(a):
    out = dict(a)
    out["bvh"], out["verts"] = a["bvh"].copy(), a["verts"].copy()
    return out


@pytest.mark.parametrize("base,builder", [("soup", "library"), ("soup", "median_permuted"), ("cornell", "loose")])
def test_child_box_one_ulp_outside_its_parent(built, base, builder):
    a = built[base, builder]
    pn, _ = _parents(a["bvh"])
    for c, axis, side in [(int(np.argmax(pn >= 0)), 0, "hi"), (len(pn) - 1, 2, "lo"), (len(pn) // 2, 1, "hi")]:
        m = _mutable(a)
        p = int(pn[c])
        assert p >= 0
        m["bvh"][side][c, axis] = np.nextafter(a["bvh"][side][p, axis], F(np.inf if side == "hi" else -np.inf))
        assert cs.check_contract(m) != []
        _refused(m, _lib.PT_E_SCENE, "node %d " % c, "node %d" % p)


@pytest.mark.parametrize("base,builder", [("soup", "library"), ("soup", "median_permuted"), ("subset", "chain_left")])
def test_vertex_one_ulp_outside_its_node_box(built, base, builder):
    a = built[base, builder]
    _, ptri = _parents(a["bvh"])
    for k, corner, axis, side in [(0, "v0", "x", "hi"), (len(ptri) - 1, "v2", "z", "lo"), (7, "v1", "y", "hi")]:
        m = _mutable(a)
        e, vi = int(ptri[k]), int(a["tris"][corner][k])
        ax = "xyz".index(axis)
        m["verts"][axis][vi] = np.nextafter(a["bvh"][side][e, ax], F(np.inf if side == "hi" else -np.inf))
        assert cs.check_contract(m) != []
        _refused(m, _lib.PT_E_SCENE, "triangle %d " % k, "node %d" % e)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_box_coordinate_not_finite(built, value):
    for node, side, axis in [(0, "hi", 0), (5, "lo", 1), (100, "hi", 2)]:
        m = _mutable(built["soup", "library"])
        m["bvh"][side][node, axis] = value
        _refused(m, _lib.PT_E_SCENE, "node %d " % node, "finite")


def test_understated_depth(built):
    for key in [("soup", "library"), ("soup", "median"), ("subset", "chain_right"), ("cornell_spheres", "permuted")]:
        a = dict(built[key])
        d = cs.true_depth(a["bvh"])
        a["bvh_depth"] = d - 1
        _refused(a, _lib.PT_E_SCENE, "bvh_depth is %d" % (d - 1), "%d levels" % d)
        a["bvh_depth"] = 0
        _refused(a, _lib.PT_E_SCENE, "bvh_depth is 0")


def test_true_depth_64_is_too_deep_whatever_the_field_says(bases):
    for lean in ("left", "right"):
        a = cs.chain(cs.soup_subset(bases["soup"], 64), lean)
        assert cs.true_depth(a["bvh"]) == 64
        a["bvh_depth"] = 63
        _refused(a, _lib.PT_E_BVH_DEPTH, "64 levels")
        a["bvh_depth"] = 64
        _refused(a, _lib.PT_E_BVH_DEPTH)
    ok = cs.chain(cs.soup_subset(bases["soup"], 63), "left")                # depth 63, the largest: accepted
    h, rc, msg = cs.ArrayScene(ok).create()
    if h:
        _lib.lib().pt_destroy(h)
    assert rc in (_lib.PT_OK, _lib.PT_E_NODEV), msg


def test_structural_refusals_still_hold(built):
    """What check_bvh refused before: a leaf reached twice, a child out of range, a cycle."""
    a = built["soup", "library"]
    m = _mutable(a)
    leaf = int(m["bvh"]["left"][-1]) if int(m["bvh"]["left"][-1]) & cs.LEAF else int(m["bvh"]["right"][-1])
    m["bvh"]["left"][-1] = m["bvh"]["right"][-1] = leaf
    _refused(m, _lib.PT_E_SCENE, "leaf")
    m = _mutable(a)
    m["bvh"]["left"][3] = len(a["bvh"])
    _refused(m, _lib.PT_E_SCENE, "out of range")
    m = _mutable(a)
    m["bvh"]["left"][3] = 0
    _refused(m, _lib.PT_E_SCENE)
