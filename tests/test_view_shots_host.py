"""The shots the oriented-camera GPU tests render (view_ref.SHOTS_EXTRA, view_ref.far_pose), checked on the reference
alone: each shot sees the scene, each non-symmetric shot tells a transposed basis, a swapped film and a mirrored right
axis from the right one, the far poses lie where they are meant to, and the host's pt_camera_ray_view makes the rays
of the restatement.  No device."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
import oracle
import view_ref

F = np.float32
W, H, SPP = 12, 8, 2
POS = (0.0, 1.0, 3.0)
SHOTS = dict(view_ref.SHOTS_EXTRA, generic=(POS, 1.0, 3.0, view_ref.generic(POS)))
FAR_M = [100.0, 128.0, float(np.nextafter(F(128), F(np.inf))), 200.0, 2e4]
EXTENT = 2.0                     # of cornell and cornell_blob: the fast walk's bound is 64 extents = 128


def _view(v):
    return pt.make_view(v[0], v[1], v[2], v[3])


def _rcam(shot, radius=0.0, w=W, h=H):
    pos, dist, focal, _ = shot
    return (tuple(pos), dist, focal, radius, w, h)


@pytest.fixture(scope="module")
def cornell():
    return oracle.OracleScene(load_scene("cornell").arrays())


@pytest.fixture(scope="module")
def blob():
    return oracle.OracleScene(load_scene("cornell_blob").arrays())


def _lit(img):
    return int(np.count_nonzero(np.asarray(img).max(axis=2) > 0))


def _changed(a, b):
    """Pixels of two images that differ in any bit."""
    return int(np.count_nonzero((np.asarray(a).view(np.uint64) != np.asarray(b).view(np.uint64)).any(axis=2)))


def _pixel_rays(rcam, view, lens=False, u1=None, u2=None):
    w, h = rcam[4], rcam[5]
    ys, xs = np.mgrid[0:h, 0:w]
    return view_ref.rays(rcam, view, xs.reshape(-1), ys.reshape(-1), lens, u1, u2)


def _primary(osc, rcam, view):
    return oracle.trace_batch(osc, *_pixel_rays(rcam, view))[0]


# ---- every shot is a valid view that sees the scene (or, for `away`, nothing of it)
def test_every_shot_is_a_valid_view():
    L = _lib.lib()
    for name, shot in list(SHOTS.items()) + [("far_%g" % m, view_ref.far_pose(m)) for m in FAR_M]:
        assert L.pt_view_validate(C.byref(_view(shot[3]))) == 0, (name, L.pt_last_error())
    # `slack` sits at nine tenths of the limit: the validated terms are the squared lengths minus 1
    r, u, _, _ = SHOTS["slack"][3]
    rr = float(np.dot(np.float64(r), np.float64(r))) - 1.0
    uu = float(np.dot(np.float64(u), np.float64(u))) - 1.0
    assert 8.9e-4 < rr < 9.1e-4 and -9.1e-4 < uu < -8.9e-4
    # (scaling the vectors themselves by 1 +- 9e-4 doubles the terms to 1.8e-3, which is refused)
    g = view_ref.generic(POS)
    bad = pt.make_view([c * (1 + 9e-4) for c in g[0]], [c * (1 - 9e-4) for c in g[1]], g[2])
    assert L.pt_view_validate(C.byref(bad)) == pt.PT_E_INVALID


def test_fov_shot_is_look_at_with_vfov():
    pos, dist, focal, v = SHOTS["fov"]
    for w, h in ((24, 16), (12, 8)):
        cam = pt.make_camera(pos, dist, focal, 0.0, w, h)
        got = pt.look_at(pos, (0.3, 0.7, -0.2), (0.1, 1.0, 0.05), vfov=35, cam=cam)
        assert bytes(got) == bytes(_view(v))
    assert v[3][0] != v[3][1]


@pytest.mark.parametrize("name", sorted(SHOTS))
def test_shot_sees_the_scene(cornell, name):
    shot = SHOTS[name]
    img, cnt = view_ref.render(cornell, _rcam(shot), shot[3], SPP, return_counters=True)
    if name != "away":
        assert _lit(img) > W * H // 4, (name, _lit(img))
        return
    assert not img.any()
    # Every camera ray misses, pinhole and through the lens.  (The oracle's `traces` says nothing here: the reference
    # integrator goes on tracing a path whose weight a miss has zeroed, so it is the same for every shot.)
    assert (_primary(cornell, _rcam(shot), shot[3]) == -1).all()
    rng = np.random.default_rng(5)
    u1, u2 = rng.random(W * H, dtype=F), rng.random(W * H, dtype=F)
    o, d = _pixel_rays(_rcam(shot, 0.05), shot[3], True, u1, u2)
    assert (oracle.trace_batch(cornell, o, d)[0] == -1).all()
    assert cnt["traces"] >= W * H * SPP
    lens = view_ref.render(cornell, _rcam(shot, 0.05), shot[3], SPP)
    assert not lens.any()


# ---- the mistakes a kernel could make with a view, each visible in the reference
def _transposed(v):
    m = np.array([v[0], v[1], v[2]], dtype=np.float64).T
    return (tuple(m[0]), tuple(m[1]), tuple(m[2]), v[3])


def _film_swapped(v):
    return (v[0], v[1], v[2], (v[3][1], v[3][0]))


def _right_negated(v):
    return (tuple(-float(c) for c in v[0]), v[1], v[2], v[3])


MISTAKES = {"transposed": _transposed, "film_swapped": _film_swapped, "right_negated": _right_negated}


# (a square film is its own swap: that mistake can show only in the shots with another film)
MISTAKEN = [(n, k) for n in ("generic", "slack", "wide", "fov") for k in sorted(MISTAKES)
            if k != "film_swapped" or SHOTS[n][3][3][0] != SHOTS[n][3][3][1]]


@pytest.mark.parametrize("name,mistake", MISTAKEN)
def test_a_mistaken_view_changes_the_image(cornell, name, mistake):
    shot = SHOTS[name]
    view = shot[3]
    good = view_ref.render(cornell, _rcam(shot), view, SPP)
    bad = view_ref.render(cornell, _rcam(shot), MISTAKES[mistake](view), SPP)
    assert _changed(good, bad) > W * H // 4, (name, mistake, _changed(good, bad))


@pytest.mark.parametrize("mistake", ["transposed", "right_negated"])
def test_a_mistaken_view_changes_the_far_pose(blob, mistake):
    """far_pose(100) looks at the box from outside, over its left wall: most of what it sees is the outside of the
    walls, which integrator 0 leaves black (3 of its 96 pixels are lit) and integrator 1 does not (50).  Integrator
    1's image changes in more than a quarter of the pixels; integrator 0's changes, which is what a bit-exact
    comparison needs; and the primary hits, which the feature buffers are compared on, change in more than a quarter."""
    shot = view_ref.far_pose(100.0)
    view = shot[3]
    wrong = MISTAKES[mistake](view)
    good = view_ref.render(blob, _rcam(shot), view, SPP, integrator=1)
    bad = view_ref.render(blob, _rcam(shot), wrong, SPP, integrator=1)
    assert _changed(good, bad) > W * H // 4, (mistake, _changed(good, bad))
    good = view_ref.render(blob, _rcam(shot), view, SPP)
    bad = view_ref.render(blob, _rcam(shot), wrong, SPP)
    assert _changed(good, bad) > 0
    a, b = _primary(blob, _rcam(shot), view), _primary(blob, _rcam(shot), wrong)
    assert int(np.count_nonzero(a != b)) > W * H // 4, (mistake, int(np.count_nonzero(a != b)))


# ---- the far poses
@pytest.mark.parametrize("m", FAR_M, ids=lambda m: "%.9g" % m)
def test_far_pose(blob, m):
    """The largest coordinate is -x = -m, on either side of 64 extents = 128.  The pose sees the box from outside
    over its left wall: the camera rays hit it in more than a quarter of the pixels.  Integrator 1's reference lights
    more than a quarter; integrator 0's only the few that look through the open front (the outside of the walls is
    black to it), and nothing where the camera ray misses."""
    shot = view_ref.far_pose(m)
    pos = shot[0]
    assert pos[0] == -float(F(m)) and max(abs(c) for c in pos) == float(F(m))
    assert (float(F(m)) <= 64.0 * EXTENT) == (m <= 128.0)
    hit = _primary(blob, _rcam(shot), shot[3]) >= 0
    assert int(hit.sum()) > W * H // 4, int(hit.sum())
    head = view_ref.render(blob, _rcam(shot), shot[3], SPP, integrator=1)
    assert _lit(head) > W * H // 4, _lit(head)
    img = view_ref.render(blob, _rcam(shot), shot[3], SPP)
    assert _lit(img) > 0
    assert not np.asarray(img)[~hit.reshape(H, W)].any()


def test_far_pose_lens_straddles_the_bound():
    """At m = 128 the camera sits on the bound near_camera() compares, and its basis tilts the lens disc along x: the
    lens origins of a radius-0.05 camera lie on both sides of |x| = 128."""
    shot = view_ref.far_pose(128.0)
    rng = np.random.default_rng(9)
    n = 200
    u1, u2 = rng.random(n, dtype=F), rng.random(n, dtype=F)
    o, _ = view_ref.rays(_rcam(shot, 0.05), shot[3], np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), True, u1, u2)
    x = np.abs(o[:, 0])
    assert (x > F(128)).any() and (x < F(128)).any(), (int((x > F(128)).sum()), int((x < F(128)).sum()))


# ---- the host's oriented ray is the restatement's, for every new shot and pose
def _lib_rays(cam, view, idxs, lens, u1, u2):
    L = _lib.lib()
    o, d = _lib.Vec3(), _lib.Vec3()
    out_o, out_d = np.empty((len(idxs), 3), dtype=F), np.empty((len(idxs), 3), dtype=F)
    for i, idx in enumerate(idxs):
        L.pt_camera_ray_view(C.byref(cam), C.byref(view), int(idx), int(lens), float(u1[i]), float(u2[i]), C.byref(o),
                             C.byref(d))
        out_o[i] = (o.x, o.y, o.z)
        out_d[i] = (d.x, d.y, d.z)
    return out_o, out_d


@pytest.mark.parametrize("name", sorted(view_ref.SHOTS_EXTRA) + ["far_%.9g" % m for m in FAR_M])
def test_camera_ray_view_equals_the_restatement(name):
    shot = view_ref.far_pose(float(name[4:])) if name.startswith("far_") else view_ref.SHOTS_EXTRA[name]
    w, h = 24, 16
    xs = np.array([0, w - 1, 0, w - 1, w // 2], dtype=np.uint32)
    ys = np.array([0, 0, h - 1, h - 1, h // 2], dtype=np.uint32)
    idxs = [view_ref.morton(int(x), int(y)) for x, y in zip(xs, ys)]
    rng = np.random.default_rng(13)
    u1, u2 = rng.random(len(xs), dtype=F), rng.random(len(xs), dtype=F)
    for radius, lens in ((0.0, False), (0.05, False), (0.05, True)):
        cam = pt.make_camera(shot[0], shot[1], shot[2], radius, w, h)
        o, d = _lib_rays(cam, _view(shot[3]), idxs, lens, u1, u2)
        ro, rd = view_ref.rays(_rcam(shot, radius, w, h), shot[3], xs, ys, lens, u1, u2)
        assert view_ref.same_bits(o, ro) == 0 and view_ref.same_bits(d, rd) == 0, (name, radius, lens)
        assert np.isfinite(d).all() and np.isfinite(o).all()
