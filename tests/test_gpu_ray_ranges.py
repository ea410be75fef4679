"""pt_trace, pt_trace_counts, pt_render_features and plain renders for rays the integrator never makes itself:
origins far outside the scene (raysets.far_sets), rays at the bounds of the fast walk's Markstein ranges
(raysets.range_edge_sets), scenes one float on either side of the per-scene range, and far cameras.  Every
comparison is (triangle, closestT) or the image bit for bit against the CPU oracle, on the render path's walk
and on the reference BVH's.  tests/test_ray_ranges_host.py shows on the CPU that the far sets hold rays whose
hit a box test without an origin bound loses."""
import os

import numpy as np
import pytest

from conftest import load_scene
from raysets import COORD_HI, COORD_LO, far_sets, range_edge_sets, ray_sets, regular_edge_sets
from test_gpu_random_scenes import write_soup

import cudapathtracer_amd as pt

import denoise_ref

pytestmark = pytest.mark.gpu

SEED = 5
N_FAR = 200000
N_EDGE = 20000
F = np.float32


def _mismatches(r, osc, sets):
    """{(set, reference_bvh): rays whose (tri, t) differ from the oracle's}, the non-zero entries only."""
    import oracle
    bad = {}
    for k, (o, d) in sets.items():
        etri, et = oracle.trace_batch(osc, o, d)
        for ref in (False, True):
            tri, t = r.trace(o, d, reference_bvh=ref)
            n = int(np.count_nonzero((tri != etri) | (t.view(np.uint32) != et.view(np.uint32))))
            print("%-22s reference_bvh=%d  rays %d  oracle hits %d  differing %d"
                  % (k, ref, len(o), int(np.count_nonzero(etri >= 0)), n))
            if n:
                bad[(k, ref)] = n
    return bad


@pytest.fixture(scope="module", params=["cornell_blob", "soup"])
def small(request, tmp_path_factory):
    import oracle
    if request.param == "soup":
        d = tmp_path_factory.mktemp("soup_ranges")
        s = pt.Scene()
        s.load_obj(write_soup(str(d), 11), mtl_basepath=str(d) + "/")
        s.build_bvh()
    else:
        s = load_scene("cornell_blob")
    a = s.arrays()
    with pt.Renderer(s, 0) as r:
        yield a, oracle.OracleScene(a), r


def test_far_origins_small_scenes(small):
    """Before pt_trace checked the origin per ray (ray_regular) the BVH4 walk returned, of 200 000 rays each at
    1e3 / 1e4 / 5e4 / just below 2^20: cornell_blob 0 / 14 / 112 / 5795 and soup 0 / 1 / 10 / 429 results that
    differ from the oracle's; the reference-BVH walk none."""
    a, osc, r = small
    bad = _mismatches(r, osc, far_sets(a, N_FAR, SEED))
    assert not bad, bad


def test_range_edges_small_scenes(small):
    """Before ray_regular bounded the direction's length, the soup's dir_scale sets differed in 3 (mixed) and 1
    (runs) rays: directions scaled by 2^20, 2^44 and 2^45 whose oracle hit is one of the soup's zero-area
    triangles -- |a| >= 0.00001 no longer rejects those at such a scale, and their "hit" lies outside every box."""
    a, osc, r = small
    bad = _mismatches(r, osc, range_edge_sets(a, N_EDGE, SEED))
    assert not bad, bad


def test_regular_ray_bounds_small_scenes(small):
    """Both sides of the two bounds at which pt_trace changes walks (64 extents, |d|^2 = 1 + 2^-10)."""
    a, osc, r = small
    bad = _mismatches(r, osc, regular_edge_sets(a, N_EDGE, SEED))
    assert not bad, bad


def test_far_origins_standin(standin_scene):
    """A tree too large for LDS: the walk's node reads come from memory.  (Without the per-ray origin check, of
    20 000 rays each: 0 / 3 / 41 / 1234 differing.)"""
    import oracle
    a = standin_scene.arrays()
    with pt.Renderer(standin_scene, 0) as r:
        bad = _mismatches(r, oracle.OracleScene(a), far_sets(a, 20000, SEED))
    assert not bad, bad


def test_trace_counts_far_origins(small):
    """The counting build of the batched trace (pt_trace_counts) on the 5e4 rung: trace's results."""
    import oracle
    a, osc, r = small
    o, d = far_sets(a, N_FAR, SEED)["far_50000"]
    etri, et = oracle.trace_batch(osc, o, d)
    for ref in (False, True):
        tri, t = r.trace(o, d, reference_bvh=ref)
        ctri, ct, counts, _ = r.trace_counts(o, d, reference_bvh=ref)
        n = int(np.count_nonzero((ctri != etri) | (ct.view(np.uint32) != et.view(np.uint32))))
        print("trace_counts reference_bvh=%d differing from the oracle %d" % (ref, n))
        assert n == 0, (ref, n)
        assert np.array_equal(ctri, tri) and np.array_equal(ct.view(np.uint32), t.view(np.uint32)), ref
        assert counts.sum() > 0


# ---------------------------------------------------------------- scene_fast, one float either side
def _outlier_scene(dirpath, x):
    """cornell_blob plus one small triangle above the box with the coordinate x (written with 9 digits: exact)."""
    p = os.path.join(dirpath, "outlier.obj")
    with open(os.path.join(dirpath, "outlier.mtl"), "w") as fh:
        fh.write("newmtl grey\nKd 0.5 0.5 0.5\n")
    with open(p, "w") as fh:
        fh.write("mtllib outlier.mtl\nusemtl grey\nv %.9g 2.5 0.25\nv 0.25 2.5 0.25\nv 0.25 2.5 0.5\nf 1 2 3\n" % float(x))
    s = load_scene("cornell_blob", build_bvh=False)
    s.load_obj(p, mtl_basepath=dirpath + "/")
    s.build_bvh()
    return s


FLIPS = [("2^20", COORD_HI, True), ("above 2^20", np.nextafter(COORD_HI, F(np.inf)), False),
         ("2^-50", COORD_LO, True), ("below 2^-50", np.nextafter(COORD_LO, F(0)), False),
         ("denormal", F(1e-40), False)]


@pytest.mark.parametrize("label,x,fast", FLIPS, ids=[f[0] for f in FLIPS])
def test_scene_range_flip(tmp_path, label, x, fast):
    """One vertex coordinate at a bound of the per-scene range (fast walk) and one float outside it (every ray
    on the exact slow walk): pt_trace and both integrators equal the oracle either way, and the renders' slow-ray
    counter (pt_stats.accel_fallbacks) says which walk ran."""
    import oracle
    s = _outlier_scene(str(tmp_path), x)
    a = s.arrays()
    vx = a["verts"]["x"]
    assert np.count_nonzero(vx.view(np.uint32) == F(x).view(np.uint32)) == 1, "the coordinate arrived exactly"
    m = np.abs(np.stack([a["verts"]["x"], a["verts"]["y"], a["verts"]["z"]]))
    in_range = bool(((m == 0) | ((m >= COORD_LO) & (m <= COORD_HI))).all())
    assert in_range == fast
    osc = oracle.OracleScene(a)
    o, d = ray_sets(load_scene("cornell_blob").arrays(), 20000, SEED)["interior"]
    w, h, spp = 24, 16, 3
    cam = pt.make_camera(width=w, height=h, pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0)
    ocam = oracle.camera((0.0, 1.0, 3.0), 1.0, 3.0, 0.0, w, h)
    with pt.Renderer(s, 0) as r:
        bad = _mismatches(r, osc, {"interior": (o, d)})
        assert not bad, bad
        for integ in (0, 1):
            img, st = r.render(cam, w, h, spp, bounces=3, integrator=integ)
            ref, cnt = oracle.render(osc, ocam, w, h, spp, 3, integ, 1234)
            diff = int(np.count_nonzero(img.view(np.uint32) != ref.astype(F).view(np.uint32)))
            print("%s integrator %d: differing values %d, rays_traced %d, accel_fallbacks %d"
                  % (label, integ, diff, st["rays_traced"], st["accel_fallbacks"]))
            assert diff == 0, (integ, diff)
            assert st["rays_reference"] == cnt["traces"]
            assert np.count_nonzero(img) > 0
            if fast:    # almost none (the bound test_gpu_parity.py sets for its scenes)
                assert st["accel_fallbacks"] <= max(10, st["rays_traced"] // 10000)
            else:
                assert st["accel_fallbacks"] == st["rays_traced"]


# ---------------------------------------------------------------- far cameras
def _far_camera(z, w, h):
    """On the +z axis at distance z, looking down -z like the standard camera (0, 1, 3), with the field of view
    narrowed so that the box still fills the frame: focal_length = z, dist_from_film = z / 3."""
    kw = dict(pos=(0.0, 1.0, float(z)), dist_from_film=float(z) / 3.0, focal_length=float(z), radius=0.0)
    import oracle
    return (pt.make_camera(width=w, height=h, **kw),
            oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], 0.0, w, h))


@pytest.fixture(scope="module")
def blob():
    import oracle
    s = load_scene("cornell_blob")
    a = s.arrays()
    with pt.Renderer(s, 0) as r:
        yield a, oracle.OracleScene(a), r


# the scene's extent is 2: 100 lies inside 64 extents (the render path's own walk), 200 just beyond, 2e4 far beyond
@pytest.mark.parametrize("z", [100.0, 200.0, 2e4])
@pytest.mark.parametrize("integ", [0, 1])
def test_far_camera_render(blob, integ, z):
    import oracle
    a, osc, r = blob
    w, h, spp = 24, 16, 3
    cam, ocam = _far_camera(z, w, h)
    ref, cnt = oracle.render(osc, ocam, w, h, spp, 3, integ, 1234)
    ref32 = ref.astype(F)
    assert np.count_nonzero(ref32.max(axis=2) > 0) > w * h // 4
    for flags in (0, pt.PT_FLAG_REFERENCE_BVH):
        img, st = r.render(cam, w, h, spp, bounces=3, integrator=integ, flags=flags)
        diff = int(np.count_nonzero(img.view(np.uint32) != ref32.view(np.uint32)))
        print("z %g integrator %d flags %d: differing values %d" % (z, integ, flags, diff))
        assert diff == 0, (flags, diff)
        assert st["rays_reference"] == cnt["traces"]


@pytest.mark.parametrize("z", [100.0, 200.0, 2e4])
def test_far_camera_features(blob, z):
    import oracle
    a, osc, r = blob
    w, h = 37, 19
    cam, _ = _far_camera(z, w, h)
    ref = denoise_ref.features_ref(a, cam, w, h, lambda o, d: oracle.trace_batch(osc, o, d))
    assert np.count_nonzero(ref["prim"] >= 0) > w * h // 4
    got = r.features(cam, w, h)
    assert got.tobytes() == ref.tobytes(), int(np.count_nonzero(got != ref))
