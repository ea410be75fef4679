"""Light-list sizes and sphere scenes on every render path, GPU against the oracle, bit for bit.

The shading code branches on two counts (pt_render.hip).  kLdsLights = 5: with fewer lights both wavefront
kernels stage the light records (integrator 1 also each light's normal and material) in LDS, with 5 or more
they read them from memory.  kMaxProbeEmitters = 4: with at most 4 emissive triangles and no spheres the
last-bounce light probe runs; more emitters, any sphere or PT_NO_LIGHT_PROBE switch it off.  The cases below
(emissive triangles, spheres, emissive spheres) straddle both constants by more than one, and every case
asserts the counts it was built for, so a test pins the regime it names.  With spheres the kernels also run
apply_spheres after every walk, drop the merged shading record, and carry sphere ids through the shared
primary-hit word of split pixels."""
import os

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

import denoise_ref
import light_scenes as ls

pytestmark = pytest.mark.gpu

CAM = dict(pos=(0.0, 1.0, 3.0), dist_from_film=1.0, focal_length=3.0, radius=0.0)
W, H, SPP, SEED = 32, 24, 4, 1234

# name: (emissive triangles, spheres, emissive spheres, scene seed, add_random_spheres options).  Odd seeds make
# triangle 0 an emitter.  The seeds are the first at which the oracle's image has non-zero pixels at every setting
# used below (bounces = 1 needs an emitter in view).
CASES = {
    "t0": (0, 0, 0, 100, {}),                                  # no lights
    "t1": (1, 0, 0, 103, {}),                                  # probe with one emitter
    "t3": (3, 0, 0, 100, {}),                                  # probe: degenerate, duplicate and occluded emitters
    "t4": (4, 0, 0, 101, {}),                                  # last staged count, last probe count
    "t5": (5, 0, 0, 103, {}),                                  # first unstaged, probe off
    "t9": (9, 0, 0, 100, {}),                                  # unstaged, probe off
    "t40": (40, 0, 0, 100, {}),                                # many lights
    "t4s3": (4, 3, 0, 100, {}),                                # probe off because of spheres; staged
    "t3s6e1": (3, 6, 1, 101, {}),                              # 4 lights staged, one a sphere
    "t3s6e2": (3, 6, 2, 100, {}),                              # 5 lights unstaged, sphere lights among them
    "t40s12e3": (40, 12, 3, 101, {}),                          # many lights with sphere lights
    "shell": (0, 41, 3, 100, dict(shell=True)),                # spheres only, the camera inside sphere 0
    "s8e6": (0, 8, 6, 100, dict(sphere0_emissive=True)),       # spheres only, unstaged
    "s8e1first": (0, 8, 1, 100, dict(sphere0_emissive=True)),  # the "nothing picked" record (sphere 0) is the light
    "s8e1": (0, 8, 1, 101, {}),                                # ... and is not
}
EXTRA = ["t3", "t4", "t5", "t3s6e2", "shell"]
FLAGS = [0, pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH,
         pt.PT_FLAG_NO_DEAD_PATH_SKIP | pt.PT_FLAG_NO_PRIMARY_CACHE, pt.PT_FLAG_COUNT]


class Case:
    """One scene, its renderer and its oracle images (computed once per configuration)."""

    def __init__(self, name, dirpath):
        self.name = name
        self.n_emissive, self.n_spheres, self.n_sphere_lights, seed, opts = CASES[name]
        s = pt.Scene()
        if self.n_emissive or not self.n_spheres:
            p = ls.write_lit_soup(dirpath, seed, self.n_emissive)
            s.load_obj(p, mtl_basepath=dirpath + "/")
        if self.n_spheres:
            ls.add_random_spheres(s, seed, self.n_spheres, self.n_sphere_lights, **opts)
        s.build_bvh()
        self.scene = s
        self.arrays = s.arrays()
        self.renderer = pt.Renderer(s, 0)
        self._ref = {}
        import oracle
        self.oracle = oracle
        self.osc = oracle.OracleScene(self.arrays)

    def close(self):
        self.renderer.close()

    def check_counts(self):
        a = self.arrays
        assert len(a["lights"]) == self.n_emissive + self.n_sphere_lights
        assert len(a["spheres"]) == self.n_spheres
        emis = int(np.count_nonzero(a["mats"]["emission"][a["tris"]["mat"], 0] != 0)) if len(a["tris"]) else 0
        assert emis == self.n_emissive

    @property
    def lit(self):
        return self.n_emissive + self.n_sphere_lights > 0

    def ref(self, integ, bounces, w=W, h=H, spp=SPP, radius=0.0):
        k = (integ, bounces, w, h, spp, radius)
        if k not in self._ref:
            ocam = self.oracle.camera(CAM["pos"], CAM["dist_from_film"], CAM["focal_length"], radius, w, h)
            img, cnt = self.oracle.render(self.osc, ocam, w, h, spp, bounces, integ, SEED)
            img.setflags(write=False)
            self._ref[k] = (img, cnt)
        return self._ref[k]

    def check(self, img, st, integ, bounces, w=W, h=H, spp=SPP, radius=0.0, order=0):
        """img (and st, unless None) against the oracle; finite; non-zero pixels."""
        ref, cnt = self.ref(integ, bounces, w, h, spp, radius)
        ref32 = ref.astype(np.float32)
        if order:
            ref32 = _morton(ref32)
        diff = int(np.count_nonzero(img.view(np.uint32) != ref32.view(np.uint32)))
        assert diff == 0, (self.name, integ, bounces, diff)
        if st is not None:
            assert st["rays_reference"] == cnt["traces"]
            assert st["samples"] == w * h * spp
        assert np.isfinite(img).all()
        # Integrator 0 adds emission only where emission[0] != 0 (kernel.cu:453): with no such material in the
        # scene its image is zero in every pixel, which is then the assertion.  Integrator 1 adds the camera
        # hit's emission unconditionally, so the Ke 0 5 5 triangles show.
        if self.lit or integ == 1:
            assert np.count_nonzero(img) > 0
        else:
            assert not img.any()


def _cam(w=W, h=H, radius=0.0):
    return pt.make_camera(width=w, height=h, **dict(CAM, radius=radius))


def _morton(a):
    h, w = a.shape[:2]
    out = np.zeros((h * w,) + a.shape[2:], dtype=a.dtype)
    for y in range(h):
        for x in range(w):
            out[pt.morton_pxl_to_i(x, y)] = a[y, x]
    return out


def _bounces(integ):
    # the probe acts on bounce D - 1: with D = 1 that is the camera ray, next to the primary-hit memo
    return (3, 1, 2) if integ == 0 else (3,)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp(request.param)))
    yield c
    c.close()


@pytest.fixture(scope="module", params=EXTRA)
def xcase(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp("x" + request.param)))
    yield c
    c.close()


@pytest.fixture(scope="module", params=["t3", "t4", "t5"])
def probe_case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp("p" + request.param)))
    yield c
    c.close()


# ---------------------------------------------------------------- every case, every traversal mode
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "f%x" % f)
@pytest.mark.parametrize("integ", [0, 1])
def test_render_matches_the_oracle(case, integ, flags):
    case.check_counts()
    for bounces in _bounces(integ):
        img, st = case.renderer.render(_cam(), W, H, SPP, bounces=bounces, integrator=integ, flags=flags)
        case.check(img, st, integ, bounces)
        if flags & pt.PT_FLAG_COUNT and len(case.arrays["tris"]):
            assert st["node_tests"] > 0


# ---------------------------------------------------------------- the five cases in depth
@pytest.mark.parametrize("integ", [0, 1])
def test_lens_camera(xcase, integ):
    xcase.check_counts()
    for bounces in _bounces(integ):
        img, st = xcase.renderer.render(_cam(radius=0.05), W, H, SPP, bounces=bounces, integrator=integ)
        xcase.check(img, st, integ, bounces, radius=0.05)


@pytest.mark.parametrize("integ", [0, 1])
def test_no_light_probe_renders_the_same_bits(probe_case, monkeypatch, integ):
    """PT_NO_LIGHT_PROBE=1 on the two cases the probe runs on: the bits of the probe-on render and the oracle.
    That the probe does run there, and with 5 emitters does not, shows in the traced rays: a probe that finds no
    emitter ends the path without a trace.  (Whole-pixel units, PT_WF_CHUNKS=1, make that count repeatable: the
    chunks of a split pixel race for its primary hit.)"""
    c = probe_case
    c.check_counts()
    assert 0 < c.n_emissive and c.n_spheres == 0
    probe_on = c.n_emissive <= 4                            # kMaxProbeEmitters
    monkeypatch.setenv("PT_WF_CHUNKS", "1")
    with pt.Renderer(c.scene, 0) as r1:
        monkeypatch.setenv("PT_NO_LIGHT_PROBE", "1")
        with pt.Renderer(c.scene, 0) as r2:
            for bounces in _bounces(integ):
                on, st_on = r1.render(_cam(), W, H, SPP, bounces=bounces, integrator=integ)
                off, st_off = r2.render(_cam(), W, H, SPP, bounces=bounces, integrator=integ)
                dflt, _ = c.renderer.render(_cam(), W, H, SPP, bounces=bounces, integrator=integ)
                assert on.tobytes() == off.tobytes() == dflt.tobytes()
                assert st_on["rays_reference"] == st_off["rays_reference"]
                c.check(off, st_off, integ, bounces)
                print(c.name, integ, bounces, "rays traced, probe on / off:", st_on["rays_traced"], st_off["rays_traced"])
                if integ == 0 and probe_on and bounces == 1:
                    # (the camera ray is traced by start_sample, which does not probe: measured equal)
                    assert st_on["rays_traced"] <= st_off["rays_traced"]
                elif integ == 0 and probe_on:
                    assert st_on["rays_traced"] < st_off["rays_traced"]
                else:                                       # (integrator 1 has no probe)
                    assert st_on["rays_traced"] == st_off["rays_traced"]


@pytest.mark.parametrize("env", [{"PT_WF_CHUNKS": "3"}, {"PT_WF_TAIL_NPIX": "100"}],
                         ids=lambda e: ",".join("%s=%s" % (k[6:], v) for k, v in e.items()))
@pytest.mark.parametrize("integ", [0, 1])
def test_split_units(xcase, monkeypatch, integ, env):
    """Sample-chunk units (every pixel in 3 chunks of 9 spp) and a split tail of 100 pixel slots: the chunks of
    a pixel share its primary hit, with spheres a sphere id."""
    xcase.check_counts()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pt.Renderer(xcase.scene, 0) as r2:
        img, st = r2.render(_cam(), W, H, 9, bounces=3, integrator=integ)
    xcase.check(img, st, integ, 3, spp=9)
    assert st["split_pixels"] > 0 and st["work_units"] > st["split_pixels"]


def test_tile_kernel_head_integrator(xcase, monkeypatch):
    xcase.check_counts()
    monkeypatch.setenv("PT_HEAD_WF", "0")
    with pt.Renderer(xcase.scene, 0) as r2:
        img, st = r2.render(_cam(), W, H, SPP, bounces=3, integrator=1)
    xcase.check(img, st, 1, 3)
    assert st["work_units"] == 0                            # (not the wavefront kernel)


@pytest.mark.parametrize("integ", [0, 1])
def test_three_shards_sum_to_the_image(xcase, integ):
    xcase.check_counts()
    acc = np.zeros((H, W, 3), dtype=np.float32)
    rays = 0
    for k in range(3):
        part, st = xcase.renderer.render(_cam(), W, H, SPP, bounces=3, integrator=integ, shard_index=k, shard_count=3)
        acc += part
        rays += st["rays_reference"]
    xcase.check(acc, None, integ, 3)
    assert rays == xcase.ref(integ, 3)[1]["traces"]


@pytest.mark.parametrize("integ", [0, 1])
def test_morton_order(xcase, integ):
    xcase.check_counts()
    img, st = xcase.renderer.render(_cam(32, 32), 32, 32, SPP, bounces=3, integrator=integ,
                                    pixel_order=pt.PT_ORDER_MORTON)
    xcase.check(img, st, integ, 3, w=32, h=32, order=1)


@pytest.mark.parametrize("integ", [0, 1])
def test_accumulated_passes(xcase, integ):
    """Passes of 2 + 1 + 1 samples: the image equals the one-shot render, the f64 mean the oracle's."""
    xcase.check_counts()
    rays = 0
    with xcase.renderer.accumulator(_cam(), W, H, bounces=3, integrator=integ) as acc:
        for k in (2, 1, 1):
            rays += acc.add(k)["rays_reference"]
        img, mean = acc.image(), acc.mean64()
    one, st = xcase.renderer.render(_cam(), W, H, SPP, bounces=3, integrator=integ)
    assert img.tobytes() == one.tobytes()
    ref, cnt = xcase.ref(integ, 3)
    assert mean.tobytes() == ref.tobytes()
    assert rays == cnt["traces"] == st["rays_reference"]
    xcase.check(img, None, integ, 3)


# ---------------------------------------------------------------- spheres on each tree shape
def _sphere_tree_check(s, r, cam_kw, integ, flags=0):
    import oracle
    cam = pt.make_camera(width=W, height=H, **cam_kw)
    img, st = r.render(cam, W, H, SPP, bounces=3, integrator=integ, flags=flags)
    ref, cnt = oracle.render(oracle.OracleScene(s.arrays()), oracle.camera(cam_kw["pos"], cam_kw["dist_from_film"],
                             cam_kw["focal_length"], cam_kw["radius"], W, H), W, H, SPP, 3, integ, SEED)
    assert img.tobytes() == ref.astype(np.float32).tobytes()
    assert st["rays_reference"] == cnt["traces"]
    assert np.isfinite(img).all() and np.count_nonzero(img) > 0
    return st


@pytest.mark.parametrize("lds_tree", ["1", "0"])
def test_cornell_with_spheres_lds_tree_on_and_off(monkeypatch, lds_tree):
    """Plain Cornell (a tree the LDS holds whole) plus 6 spheres, 2 emissive: node records from LDS or, with
    PT_WF_LDS_TREE=0, from memory."""
    monkeypatch.setenv("PT_WF_LDS_TREE", lds_tree)
    s = load_scene("cornell", build_bvh=False)
    ls.add_random_spheres(s, 7, 6, 2, box=((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0)))
    s.build_bvh()
    a = s.arrays()
    assert len(a["spheres"]) == 6 and len(a["lights"]) == 2 + 2
    with pt.Renderer(s, 0) as r:
        for integ in (0, 1):
            _sphere_tree_check(s, r, CAM, integ)
        st = _sphere_tree_check(s, r, CAM, 0, flags=pt.PT_FLAG_COUNT)
    assert st["node_tests"] > 0
    if lds_tree == "1":
        assert st["lds_node_tests"] == st["node_tests"]
    else:
        assert st["lds_node_tests"] < st["node_tests"]


# The stand-in's vases and plants do not scale, so every scale_tris gives a tree far beyond the LDS top; this is
# the smallest at which each of its grids still has a cell.
STANDIN_SMALL = 1.0 / 256.0


def test_standin_too_big_for_lds_with_spheres(tmp_path):
    p = scenes.write_sponza_standin(str(tmp_path), scale_tris=STANDIN_SMALL)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    ls.add_random_spheres(s, 9, 6, 2, box=((-2.5, 0.5, 4.0), (2.5, 5.0, 11.0)), radii=(0.1, 0.5, 1.2))
    s.build_bvh()
    a = s.arrays()
    assert len(a["spheres"]) == 6 and len(a["lights"]) == 2 + 2
    with pt.Renderer(s, 0) as r:
        for integ in (0, 1):
            _sphere_tree_check(s, r, scenes.SPONZA_STANDIN_CAMERA, integ)
        st = _sphere_tree_check(s, r, scenes.SPONZA_STANDIN_CAMERA, 0, flags=pt.PT_FLAG_COUNT)
    assert 0 < st["lds_node_tests"] < st["node_tests"]      # the tree is not held whole in LDS


# ---------------------------------------------------------------- pt_trace with spheres
@pytest.fixture(scope="module", params=["shell", "t3s6e2", "s300"])
def trace_case(request, tmp_path_factory):
    if request.param == "s300":
        s = pt.Scene()
        ls.add_random_spheres(s, 300, 300, 5)
        s.build_bvh()
        with pt.Renderer(s, 0) as r:
            yield s, r, 300
    else:
        c = Case(request.param, str(tmp_path_factory.mktemp("tr" + request.param)))
        c.check_counts()
        yield c.scene, c.renderer, c.n_spheres
        c.close()


def test_pt_trace_with_spheres(trace_case):
    """Interior origins, origins inside spheres, rays leaving surfaces at t - 0.001 and silhouette rays, on both
    walks: hit ids and t bits equal the oracle's."""
    import oracle
    s, r, n_spheres = trace_case
    a = s.arrays()
    assert len(a["spheres"]) == n_spheres
    osc = oracle.OracleScene(a)
    n = 20000
    sets = ls.sphere_ray_sets(a["spheres"], n, 77)
    sets["leaving"] = ls.leaving_rays(lambda o, d: oracle.trace_batch(osc, o, d), *sets["interior"], 78)
    nt = len(a["tris"])
    for name, (o, d) in sets.items():
        etri, et = oracle.trace_batch(osc, o, d)
        assert np.count_nonzero(etri >= nt) > 100, name                   # spheres are hit
        for ref_bvh in (False, True):
            tri, t = r.trace(o, d, reference_bvh=ref_bvh)
            assert np.array_equal(tri, etri), (name, ref_bvh, int(np.count_nonzero(tri != etri)))
            assert t.tobytes() == et.tobytes(), (name, ref_bvh)


# ---------------------------------------------------------------- feature buffers
@pytest.fixture(scope="module", params=["shell", "t3s6e2"])
def feature_case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp("ft" + request.param)))
    yield c
    c.close()


def test_features_equal_host_composition(feature_case):
    """Renderer.features equals test_gpu_features.py's host composition (denoise_ref.features_ref)."""
    c = feature_case
    c.check_counts()
    cam = _cam()
    got = c.renderer.features(cam, W, H)
    ref = denoise_ref.features_ref(c.arrays, cam, W, H, c.renderer.trace)
    nt = len(c.arrays["tris"])
    assert ((ref["prim"] & ~pt.PT_FEATURE_EMISSIVE) >= nt)[ref["prim"] >= 0].any()   # spheres are seen
    assert got.tobytes() == ref.tobytes()
