"""The shading pass's guards, GPU against the oracle, bit for bit (24 x 16 pixels, 8 spp, depth 3 and 8, both
integrators, the plain wavefront kernel and an accumulator of 2 x 4 spp -- they share shade_lane).

shade_lane tests the range predicates of pt_device.h as mask arithmetic (ray_fast_m) behind the wave-uniform tests,
so that the walk state is merged behind one branch.  The inputs put lanes on both sides of each guard:
  lens_tiny_x     Cornell, a lens camera at pos.x = 2^-60 (coord_ok false): every primary ray takes the slow walk
                  while the same wave's secondary rays take the fast one -- the mixed wave in which a wrong merge
                  of the walk state or a wrong mask shows;
  pinhole_tiny_x  the same with a pinhole camera: only each pixel's first sample is slow;
  scale_2p12, scale_2p19   Cornell scaled: inside the fast range, and at its upper edge (coordinates up to 2^20);
  scale_2p24      scene_fast false: every trace takes the slow walk through shade_lane's scalar branch (the two
                  large scalings with the camera under the light, so that the frame is lit: see CASES);
  sphere_light, many_lights   tests/light_scenes.py: the sphere-light branch and the area pick over 40 lights.
"""
import os

import numpy as np
import pytest

from conftest import MODELS

import cudapathtracer_amd as pt

import light_scenes as ls

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 24, 16, 8, 1234
TINY = 2.0 ** -60


def _cornell(scale):
    s = pt.Scene()
    s.load_obj(os.path.join(MODELS, "cornell.obj"), (0, 0, 0), scale, 0, mtl_basepath=MODELS + "/")
    s.build_bvh()
    return s


def _lit(tmp, seed, n_emissive, n_spheres, n_sphere_lights):
    s = pt.Scene()
    p = ls.write_lit_soup(tmp, seed, n_emissive)
    s.load_obj(p, mtl_basepath=tmp + "/")
    if n_spheres:
        ls.add_random_spheres(s, seed, n_spheres, n_sphere_lights)
    s.build_bvh()
    return s


# name: (scene factory(tmp dir), camera position, lens radius)
CASES = {
    "lens_tiny_x": (lambda tmp: _cornell(1.0), (TINY, 1.0, 3.0), 0.05),
    "pinhole_tiny_x": (lambda tmp: _cornell(1.0), (TINY, 1.0, 3.0), 0.0),
    "scale_2p12": (lambda tmp: _cornell(2.0 ** 12), (0.0, 2.0 ** 12, 3 * 2.0 ** 12), 0.0),
    # At these two scales the box is far wider than MAX_FLOAT = 100000 (limits.h:3), and a hit with t > MAX_FLOAT - 1
    # is a miss: seen from the usual place the oracle's frame is black whatever the kernels do.  So the camera sits
    # 4096 below the ceiling light (y = 1.98 * scale, facing down) and looks along -z under it: the upper half of the
    # frame hits the light within 14000 and is lit (192 of 384 pixels in the oracle's image), the rest is dark.
    "scale_2p19": (lambda tmp: _cornell(2.0 ** 19), (0.0, 1.98 * 2.0 ** 19 - 4096.0, 16384.0), 0.0),
    "scale_2p24": (lambda tmp: _cornell(2.0 ** 24), (0.0, 1.98 * 2.0 ** 24 - 4096.0, 16384.0), 0.0),
    "sphere_light": (lambda tmp: _lit(tmp, 101, 3, 6, 1), (0.0, 1.0, 3.0), 0.0),
    "many_lights": (lambda tmp: _lit(tmp, 100, 40, 0, 0), (0.0, 1.0, 3.0), 0.0),
}
# lit pixels the oracle's image must have at least (the scaled cases: half the frame sees the light)
MIN_LIT = {"scale_2p19": 150, "scale_2p24": 150}


class Case:
    def __init__(self, name, tmp):
        import oracle
        make, self.pos, self.radius = CASES[name]
        self.name = name
        self.scene = make(tmp)
        self.arrays = self.scene.arrays()
        self.renderer = pt.Renderer(self.scene, 0)
        self.oracle = oracle
        self.osc = oracle.OracleScene(self.arrays)
        self._ref = {}

    def cam(self):
        return pt.make_camera(self.pos, 1.0, 3.0, self.radius, W, H)

    def ref(self, integ, bounces):
        k = (integ, bounces)
        if k not in self._ref:
            ocam = self.oracle.camera(self.pos, 1.0, 3.0, self.radius, W, H)
            img, _ = self.oracle.render(self.osc, ocam, W, H, SPP, bounces, integ, SEED)
            img.setflags(write=False)
            self._ref[k] = img
        return self._ref[k]


@pytest.fixture(scope="module", params=list(CASES))
def case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp(request.param)))
    yield c
    c.renderer.close()


def test_case_reaches_its_guard(case):
    """The inputs are what the docstring says: which side of coord_ok / scene_fast each case lies on."""
    a = case.arrays
    v = np.abs(np.stack([a["verts"][k] for k in "xyz"], axis=1))
    nz = v[v > 0]
    in_range = bool((nz >= np.float32(2.0 ** -50)).all() and (nz <= np.float32(2.0 ** 20)).all())
    pos = np.abs(np.float32(case.pos))
    pos_ok = bool(((pos == 0) | ((pos >= np.float32(2.0 ** -50)) & (pos <= np.float32(2.0 ** 20)))).all())
    if case.name in ("lens_tiny_x", "pinhole_tiny_x"):
        assert in_range and not pos_ok and np.float32(case.pos[0]) == np.float32(TINY)
    elif case.name == "scale_2p24":
        assert not in_range and v.max() > 2.0 ** 24
    else:
        assert in_range and pos_ok
    if case.name == "scale_2p19":
        assert 2.0 ** 19 < v.max() <= 2.0 ** 20
    if case.name == "sphere_light":
        assert len(a["spheres"]) == 6 and len(a["lights"]) == 4
    if case.name == "many_lights":
        assert len(a["lights"]) == 40 and len(a["spheres"]) == 0


@pytest.mark.parametrize("bounces", [3, 8])
@pytest.mark.parametrize("integ", [0, 1])
def test_render_and_accumulator_match_the_oracle(case, integ, bounces):
    ref = case.ref(integ, bounces)
    ref32 = ref.astype(np.float32)
    img, st = case.renderer.render(case.cam(), W, H, SPP, bounces=bounces, integrator=integ, seed=SEED)
    assert st["samples"] == W * H * SPP
    bad = int(np.count_nonzero(img.view(np.uint32) != ref32.view(np.uint32)))
    assert bad == 0, (case.name, integ, bounces, "render", bad)
    assert np.isfinite(img).all()
    assert np.count_nonzero(img.sum(axis=2)) >= MIN_LIT.get(case.name, 1)
    with case.renderer.accumulator(case.cam(), W, H, bounces=bounces, integrator=integ, seed=SEED) as acc:
        acc.add(SPP // 2)
        acc.add(SPP // 2)
        aimg, mean = acc.image(), acc.mean64()
    assert mean.tobytes() == ref.tobytes(), (case.name, integ, bounces, "accumulator mean")
    assert aimg.tobytes() == img.tobytes()
