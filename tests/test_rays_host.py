"""Renders along caller-supplied rays without a device (include/pt/pt.h, pt_render_rays*): what the restatement of the
definition (rays_ref) is worth -- over the camera's own rays it is the oracle's render except at Morton index 0, and it
discriminates --, the ray helpers of cudapathtracer_amd.rays, the classes of the test's own ray sets, and the entry
points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
from cudapathtracer_amd import rays                          # (the parent has no such module: every test here errors there)
import oracle
import rays_ref
import view_ref

F = np.float32
W, H, SPP, BOUNCES, SEED = 24, 16, 4, 3, 1234
POS = rays_ref.POS


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def osc(scene):
    return oracle.OracleScene(scene.arrays())


@pytest.fixture(scope="module")
def cam_rays():
    return rays_ref.set_camera(pt, W, H)


# ---- 1. the restatement over the camera's own rays is the oracle's render, except at Morton index 0
# (dist 3: with the other suites' camera pixel (0, 0) looks past the box and is black with either stream)
@pytest.mark.parametrize("dist", [1.0, 3.0])
@pytest.mark.parametrize("integrator", [0, 1])
def test_restatement_equals_the_oracle_except_at_morton_0(osc, integrator, dist):
    o, d = rays_ref.set_camera(pt, W, H, dist)
    got, cnt = rays_ref.render_cached("cornell/a%g" % dist, osc, o, d, W, H, SPP, BOUNCES, integrator, SEED)
    want, ocnt = oracle.render(osc, oracle.camera(POS, dist, 3.0, 0.0, W, H), W, H, SPP, BOUNCES, integrator, SEED)
    assert rays_ref.morton(0, 0) == 0
    differs = np.any(got.view(np.uint64) != want.view(np.uint64), axis=2)
    if dist == 3.0:
        assert differs[0, 0], "pixel (0, 0): the plain render draws the two quirk lens numbers per sample, this one does not"
    differs[0, 0] = False
    assert not differs.any(), np.argwhere(differs)[:5]
    assert np.count_nonzero(want) > W * H
    # the trace counts agree once pixel (0, 0)'s are taken out on both sides
    _, c0 = rays_ref.render(osc, o, d, W, H, SPP, BOUNCES, integrator, SEED, pixels=[0], return_counters=True)
    _, oc0 = oracle.render(osc, oracle.camera(POS, dist, 3.0, 0.0, W, H), W, H, SPP, BOUNCES, integrator, SEED, pixels=[0])
    assert cnt["traces"] - c0["traces"] == ocnt["traces"] - oc0["traces"]


# ---- 2. the restatement discriminates
@pytest.mark.parametrize("integrator", [0, 1])
def test_restatement_discriminates(osc, cam_rays, integrator):
    o, d = cam_rays
    ref, _ = rays_ref.render_cached("cornell/a1", osc, o, d, W, H, SPP, BOUNCES, integrator, SEED)
    # the rays of two pixels that see different things, swapped (a wall pixel and one looking at the light's rim)
    a, b = 3 * W + 2, 8 * W + 12
    o2, d2 = o.copy(), d.copy()
    o2[[a, b]] = o[[b, a]]
    d2[[a, b]] = d[[b, a]]
    sw = rays_ref.render(osc, o2, d2, W, H, SPP, BOUNCES, integrator, SEED, pixels=[a, b])
    for k in (a, b):
        assert rays_ref.same_bits(sw[k // W, k % W], ref[k // W, k % W]) > 0, k
    # one extra draw per sample shifts every stream
    rows = range(4 * W, 6 * W)
    ex = rays_ref.render(osc, o, d, W, H, SPP, BOUNCES, integrator, SEED, pixels=rows, extra_draw=True)
    changed = np.any(ex[4:6] != ref[4:6], axis=2)
    assert changed.sum() > W, changed.sum()


# ---- 3. the helpers
def test_camera_rays_equal_pt_camera_ray_view():
    L = _lib.lib()
    for view in (None, view_ref.generic(POS)):
        v = None if view is None else pt.make_view(view[0], view[1], view[2], view[3])
        for radius in (0.0, 0.05):          # (lens = 0: the radius plays no part)
            cam = pt.make_camera(POS, 1.0, 3.0, radius, 13, 7)
            o, d = rays.camera_rays(cam, v)
            assert o.shape == d.shape == (13 * 7, 3) and o.dtype == d.dtype == F
            oo, dd = _lib.Vec3(), _lib.Vec3()
            for y in range(7):
                for x in range(13):
                    L.pt_camera_ray_view(C.byref(cam), None if v is None else C.byref(v), rays_ref.morton(x, y), 0, 0.0, 0.0,
                                         C.byref(oo), C.byref(dd))
                    want = np.array((oo.x, oo.y, oo.z, dd.x, dd.y, dd.z), dtype=F)
                    assert rays_ref.same_bits(np.concatenate([o[y * 13 + x], d[y * 13 + x]]), want) == 0, (x, y)


def _len2(d):
    l2 = d[:, 0] * d[:, 0]
    l2 = l2 + d[:, 1] * d[:, 1]
    return l2 + d[:, 2] * d[:, 2]


HELPERS = {
    "camera": lambda: rays.camera_rays(pt.make_camera(POS, 1.0, 3.0, 0.0, 37, 19)),
    "camera_view": lambda: rays.camera_rays(pt.make_camera(POS, 1.0, 3.0, 0.0, 37, 19),
                                            pt.look_at(POS, (0.3, 0.5, 0.0), vfov=50.0, cam=pt.make_camera(POS, 1.0, 3.0, 0.0, 37, 19))),
    "ortho": lambda: rays.ortho_rays(POS, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.8, 1.8, 37, 19),
    "ortho_oblique": lambda: rays.ortho_rays((2.0, 3.0, 4.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 3.0, 2.0, 37, 19),
    "panorama": lambda: rays.panorama_rays((0.1, 0.9, 0.2), 64, 32),
    "panorama_1x1": lambda: rays.panorama_rays((0.1, 0.9, 0.2), 1, 1),
    "fisheye_180": lambda: rays.fisheye_rays(POS, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 180.0, 37, 19),
    "fisheye_360": lambda: rays.fisheye_rays((0.0, 1.0, 0.0), (0.0, 1.0, -1.0), (0.0, 1.0, 0.0), 360.0, 33, 33),
}


@pytest.mark.parametrize("name", sorted(HELPERS))
def test_helpers_return_finite_normalised_rays(name):
    o, d = HELPERS[name]()
    assert o.dtype == d.dtype == F and o.shape == d.shape and o.ndim == 2 and o.shape[1] == 3
    assert o.flags.c_contiguous and d.flags.c_contiguous
    assert np.isfinite(o).all() and np.isfinite(d).all()
    l2 = _len2(d)
    assert l2.dtype == F and (l2 <= rays_ref.DIR_LEN2_MAX).all() and (l2 >= F(1.0) - F(2.0 ** -10)).all()


def test_helper_geometry():
    # orthographic along -z: the direction is exactly (0, 0, -1) and every pixel has an origin of its own
    o, d = rays_ref.set_ortho(W, H)
    assert (d == np.array((0.0, 0.0, -1.0), dtype=F)).all()
    assert len({tuple(r) for r in o.tolist()}) == W * H
    assert np.allclose(o[:, 2], 3.0) and abs(float(o[:, 0].mean())) < 1e-6 and abs(float(o[:, 1].mean()) - 1.0) < 1e-6
    # the image's orientation is the camera's: pixel (0, 0) looks up and to +x
    assert o[0, 0] > 0 and o[0, 1] > 1.0
    co, cd = rays_ref.set_camera(pt, W, H)
    assert cd[0, 0] > 0 and cd[0, 1] > 0
    # the panorama covers all eight octants; its middle looks down -z, row 0 up
    po, pd = rays.panorama_rays((0.0, 1.0, 0.0), 64, 32)
    assert len({tuple(r) for r in (pd > 0).tolist()}) == 8
    mid = pd[16 * 64 + 32]
    assert mid[2] < -0.99 and pd[0, 1] > 0.99 and pd[-1, 1] < -0.99
    # the fisheye's centre looks at the target, and the inscribed circle's edge is fov / 2 off the axis
    fo, fd = rays.fisheye_rays((0.0, 1.0, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 120.0, 33, 33)
    assert fd[16 * 33 + 16][2] < -0.9999
    edge = fd[16 * 33 + 0]
    assert abs(np.degrees(np.arccos(-edge[2])) - 60.0 * (16.0 / 16.5)) < 0.1 and edge[0] > 0


# ---- 4. the test's own ray sets are what they claim to be
def test_ray_sets_have_the_classes_they_claim(scene):
    ext = rays_ref.scene_extent(scene.arrays())
    assert ext == 2.0 or 1.0 <= ext <= 4.0          # (the Cornell box)
    n = W * H
    regular_sets = {"a": rays_ref.set_camera(pt, W, H), "b": rays_ref.set_ortho(W, H), "c": rays_ref.set_panorama(W, H),
                    "d": rays_ref.set_probes(W, H), "e": rays_ref.set_mixed(pt, W, H)}
    for name, (o, d) in regular_sets.items():
        got, _ = rays_ref.classify(o, d, ext)
        assert got == dict(regular=n, irregular=0, invalid=0, first_invalid=rays_ref.NONE), name
    got, cls = rays_ref.classify(*rays_ref.set_irregular(pt, W, H), ext)
    k = (H // 2) * W + W // 2
    assert got == dict(regular=n - 2, irregular=2, invalid=0, first_invalid=rays_ref.NONE)
    assert list(np.flatnonzero(cls == 1)) == [k, k + 1]
    # set c holds the six axis directions, set d starts on the floor and points into the room, set e leaves the fast
    # walk's origin range (0 or >= 2^-50) in every third ray
    assert (regular_sets["c"][1][:6] == np.array(rays_ref.AXES, dtype=F)).all()
    assert len({tuple(r) for r in (regular_sets["c"][1] > 0).tolist()}) == 8
    assert (regular_sets["d"][0][:, 1] == F(1e-3)).all() and (regular_sets["d"][1][:, 1] > 0).all()
    e = regular_sets["e"][0][:, 0]
    assert (e[::3] == F(2.0 ** -60)).all() and (np.abs(e[::3]) < F(2.0 ** -50)).all()
    # the invalid kinds, and the edge of the direction bound
    o, d = (a.copy() for a in regular_sets["a"])
    d[7] = 0
    o[5, 1] = np.nan
    d[9, 2] = np.inf
    got, cls = rays_ref.classify(o, d, ext)
    assert got == dict(regular=n - 3, irregular=0, invalid=3, first_invalid=5) and list(np.flatnonzero(cls == 2)) == [5, 7, 9]
    edge = np.array([[np.sqrt(rays_ref.DIR_LEN2_MAX), 0, 0], [np.nextafter(np.sqrt(rays_ref.DIR_LEN2_MAX), F(2)), 0, 0],
                     [3e38, 3e38, 0], [0, -0.0, 1e-30]], dtype=F)
    got, cls = rays_ref.classify(np.zeros_like(edge), edge, ext)
    assert list(cls) == [0, 1, 1, 0]
    far = np.array([[64 * ext, 0, 0], [np.nextafter(F(64 * ext), F(1e9)), 0, 0], [0, -64 * ext, 0]], dtype=F)
    got, cls = rays_ref.classify(far, np.tile(np.array((0, 0, 1), dtype=F), (3, 1)), ext)
    assert list(cls) == [0, 1, 0]


# ---- the entry points' checks that need no device
def test_entry_points_refuse_null_arguments():
    L = _lib.lib()
    p = pt.Renderer.params(W, H, SPP)
    st = _lib.Stats()
    rc = _lib.RayClasses()
    assert C.sizeof(_lib.RayClasses) == 32
    assert L.pt_render_rays(None, C.byref(p), None, None, C.byref(st)) == _lib.PT_E_INVALID
    assert b"null" in L.pt_last_error()
    assert L.pt_render_rays_device(None, C.byref(p), None, None, None, C.byref(st)) == _lib.PT_E_INVALID
    assert L.pt_rays_classify_device(None, 0, None, None, C.byref(rc)) == _lib.PT_E_INVALID
    for name in ("pt_render_rays", "pt_render_rays_device", "pt_rays_classify_device"):
        assert name in _lib.SIGNATURES
    assert L.pt_abi_version() == 6
