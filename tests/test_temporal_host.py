"""Temporal reprojection without a device (include/pt/pt.h, pt_project_view / pt_temporal_*): the projection against
its numpy restatement (temporal_ref) in every bit, the round trip that makes the snap condition hold, the restatement
itself on oracle renders along a look-at orbit and under a still camera, and the refusals the library makes before it
needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
import oracle
import temporal_ref
import view_ref
from temporal_ref import F, TemporalRef

POS = (0.0, 1.0, 3.0)    # the Cornell camera (kernel.cu:642-648)
SIZES = [(24, 16), (37, 19)]
X = view_ref.SHOTS_EXTRA
# (pos, view): the NULL view, look-at views, a mirror, a roll, a narrow and a wide film, a field-of-view film
POSES = {
    "null": (POS, None),
    "generic": (POS, view_ref.generic(POS)),
    "orbit": temporal_ref.orbit_pose(5),
    "mirror": (X["mirror"][0], X["mirror"][3]),
    "roll90": (X["roll90"][0], X["roll90"][3]),
    "narrow": (X["narrow"][0], X["narrow"][3]),
    "wide": (X["wide"][0], X["wide"][3]),
    "fov": (X["fov"][0], X["fov"][3]),
}


def _view(v):
    return None if v is None else pt.make_view(v[0], v[1], v[2], v[3])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _lib_project(cam, view, P):
    front = np.empty(len(P), dtype=bool)
    sx, sy = np.empty(len(P), dtype=F), np.empty(len(P), dtype=F)
    for i, p in enumerate(P):
        front[i], sx[i], sy[i] = pt.project(cam, p, view)
    return front, sx, sy


# ---------------------------------------------------------------- 1. pt_project_view
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", sorted(POSES))
def test_project_view_equals_the_restatement(name, size):
    W, H = size
    pos, v = POSES[name]
    cam, rcam = pt.make_camera(pos, 1.0, 3.0, 0.0, W, H), (pos, 1.0, 3.0, 0.0, W, H)
    rng = np.random.default_rng(5 + W)
    P = (rng.normal(size=(400, 3)) * 3.0 + np.array([0.0, 1.0, 0.0])).astype(F)      # around the box, many behind the camera
    P[:8] = np.asarray(pos, dtype=F)                                                 # the camera's own position: c = 0
    P[8:16, 2] = F(pos[2])                                                           # (null view) in the camera's plane
    front, sx, sy = _lib_project(cam, _view(v), P)
    rf, rx, ry = temporal_ref.project(rcam, v, P)
    assert np.array_equal(front, rf)
    assert 40 < np.count_nonzero(front) < 360                                        # both sides of the camera
    assert np.array_equal(_bits(sx[front]), _bits(rx[front])) and np.array_equal(_bits(sy[front]), _bits(ry[front]))


def test_project_view_null_arguments():
    L = _lib.lib()
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, 24, 16)
    sx, sy = C.c_float(), C.c_float()
    P = _lib.Vec3(0.0, 1.0, 0.0)
    assert L.pt_project_view(None, None, P, C.byref(sx), C.byref(sy)) == _lib.PT_E_INVALID
    assert b"null" in L.pt_last_error()
    assert L.pt_project_view(C.byref(cam), None, P, None, C.byref(sy)) == _lib.PT_E_INVALID
    assert L.pt_project_view(C.byref(cam), None, P, C.byref(sx), None) == _lib.PT_E_INVALID
    assert L.pt_project_view(C.byref(cam), None, P, C.byref(sx), C.byref(sy)) == 1
    assert (sx.value, sy.value) == (12.0, 8.0)                                       # the target of the centre ray
    assert pt.project(cam, (0.0, 1.0, 4.0))[0] is False                             # behind the camera


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["null", "generic", "orbit", "mirror", "fov", "wide"])
def test_round_trip_lands_within_the_snap_distance(name, size):
    """Projecting o + d*t of every pixel's ray gives the pixel back to well within 1/64 pixel -- by the restatement
    alone, and by the library -- for the corner ray (px) and the ray through the footprint's centre (px + 0.5)."""
    W, H = size
    pos, v = POSES[name]
    cam, rcam = pt.make_camera(pos, 1.0, 3.0, 0.0, W, H), (pos, 1.0, 3.0, 0.0, W, H)
    rng = np.random.default_rng(9 + W)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    t = rng.uniform(0.3, 6.0, len(xs)).astype(F)
    for off in (0.0, 0.5):
        o, d = np.empty((len(xs), 3), dtype=F), np.empty((len(xs), 3), dtype=F)
        for i, (x, y) in enumerate(zip(xs, ys)):
            o[i], d[i] = pt.camera_ray(cam, view_ref.morton(int(x), int(y)), view=_view(v), jitter=(off, off))
        P = np.empty_like(o)
        for k in range(3):
            step = d[:, k] * t
            P[:, k] = o[:, k] + step                                                 # position = o + d*depth, as the features
        rf, rx, ry = temporal_ref.project(rcam, v, P)
        assert rf.all()
        ex, ey = np.abs(rx - (xs + off).astype(F)), np.abs(ry - (ys + off).astype(F))
        assert max(ex.max(), ey.max()) <= float(temporal_ref.SNAP) / 4, (name, off, ex.max(), ey.max())
        front, sx, sy = _lib_project(cam, _view(v), P[::7])
        assert front.all() and np.array_equal(_bits(sx), _bits(rx[::7])) and np.array_equal(_bits(sy), _bits(ry[::7]))


# ---------------------------------------------------------------- 2. the restatement on oracle renders
@pytest.fixture(scope="module")
def cornell():
    arrays = load_scene("cornell").arrays()
    return arrays, oracle.OracleScene(arrays)


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def test_orbit_is_closer_to_the_converged_render_than_its_last_frame(cornell):
    """8 frames of 1 spp along the look-at orbit, independent seeds: the temporal image is closer (RMSE) to the
    oracle's 2048-spp render of the last view (the committed fixture, temporal_ref.make_orbit_golden) than the last
    frame alone; a pixel the move revealed has history length 1."""
    arrays, osc = cornell
    S = temporal_ref.ORBIT_SIZE
    ref = np.load(os.path.join(GOLD, temporal_ref.ORBIT_GOLDEN))
    assert ref.shape == (S, S, 3) and ref.dtype == F
    tr = TemporalRef(S, S)
    revealed = 0
    for i in range(temporal_ref.ORBIT_FRAMES):
        pos, view = temporal_ref.orbit_pose(i)
        rcam = (pos, 1.0, 3.0, 0.0, S, S)
        img = view_ref.render(osc, rcam, view, 1, 3, 0, temporal_ref.ORBIT_SEED + i).astype(F)
        feat = temporal_ref.features_ref(arrays, rcam, view, lambda o, d: oracle.trace_batch(osc, o, d))
        out, var = tr.push(img, feat, rcam, view)
        n = tr.history_length()
        hit = feat["prim"] >= 0
        assert np.array_equal(np.isinf(var), n < 2) and np.all(var[n >= 2] >= 0)
        if i == 0:
            assert np.array_equal(_bits(out), _bits(img)) and np.all(n == 1)
        else:
            st = tr.stats
            assert st["fractional"] > S * S // 2 and st["tap_pass"] > S * S                # a real move, a real history
            assert np.all(n[~hit] == 1) and n.max() <= i + 1 + 1e-4
            assert np.count_nonzero(n[hit] > i + 0.5) > hit.sum() // 2                     # most pixels keep every frame
            # a pixel the move revealed (beside an occluder's edge: a hit none of whose taps is consistent with it)
            # starts over: history length 1, its input unchanged, its variance unknown
            fresh = hit & (n == 1)
            revealed += int(np.count_nonzero(fresh))
            assert np.count_nonzero(fresh) == hit.sum() - st["history_used"]
            assert np.array_equal(_bits(out[fresh]), _bits(img[fresh])) and np.all(np.isinf(var[fresh]))
    assert revealed > 0
    e_temporal, e_last = _rmse(out, ref), _rmse(img, ref)
    print("orbit: RMSE temporal %.5f, last frame %.5f, ratio %.4f" % (e_temporal, e_last, e_temporal / e_last))
    assert e_temporal / e_last < 1.0


@pytest.mark.parametrize("view_name", ["null", "generic"])
def test_still_camera_is_the_running_mean(cornell, view_name):
    """k pushes of k independent frames through one camera: n' = k wherever the camera ray hits, the output is the f32
    recurrence m + (x - m)/k exactly (the snap makes every pixel read itself with weight 1), and the variance is the
    restatement's formula on the recurrence of the luminance moments."""
    arrays, osc = cornell
    W, H, K = 24, 16, 5
    pos, view = POSES[view_name]
    rcam = (pos, 1.0, 3.0, 0.0, W, H)
    ocam = oracle.camera(pos, 1.0, 3.0, 0.0, W, H)
    vv = view_ref.IDENTITY if view is None else view
    feat = temporal_ref.features_ref(arrays, rcam, vv, lambda o, d: oracle.trace_batch(osc, o, d))
    hit = feat["prim"] >= 0
    assert W * H // 2 < hit.sum()
    tr = TemporalRef(W, H)
    m = np.zeros((H, W, 3), dtype=F)
    m1, m2 = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    for k in range(1, K + 1):
        if view is None:
            x = oracle.render(osc, ocam, W, H, 1, 3, 0, 100 + k)[0].astype(F)
        else:
            x = view_ref.render(osc, rcam, view, 1, 3, 0, 100 + k).astype(F)
        out, var = tr.push(x, feat, rcam, vv)
        if k > 1:
            assert tr.stats["snapped"] + tr.stats["exact"] == hit.sum() and tr.stats["fractional"] == 0
        a = F(1) / F(k)
        d = x - m
        d = d * a
        m = np.where(hit[..., None], m + d, x)
        l = temporal_ref.lum(x)
        d = (l - m1) * a
        m1 = np.where(hit, m1 + d, l)
        d = (l * l - m2) * a
        m2 = np.where(hit, m2 + d, l * l)
        n = tr.history_length()
        assert np.all(n[hit] == k) and np.all(n[~hit] == 1)
        assert np.array_equal(_bits(out), _bits(m))
        if k >= 2:
            d = m2 - m1 * m1
            want = np.where(d > 0, d, F(0)) / F(k - 1)
            assert np.array_equal(_bits(var[hit]), _bits(want[hit])) and np.all(np.isinf(var[~hit]))
        else:
            assert np.all(np.isinf(var))


def test_history_cap_turns_the_mean_into_an_exponential_average():
    """max_history = 2: from the third push on n' stays 2 and the output is h + (x - h)/2."""
    W, H = 5, 3
    rcam = (POS, 1.0, 3.0, 0.0, W, H)
    feat = np.zeros((H, W), dtype=pt.FEATURE)
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = view_ref.rays(rcam, view_ref.IDENTITY, xs.reshape(-1), ys.reshape(-1), False)
    feat["position"] = (o + d * F(2.0)).reshape(H, W, 3)
    feat["normal"] = (0, 0, 1)
    feat["depth"] = 2.0
    feat["prim"] = 7
    rng = np.random.default_rng(2)
    tr = TemporalRef(W, H, max_history=2)
    prev = None
    for k in range(4):
        x = rng.uniform(0, 4, (H, W, 3)).astype(F)
        out, _ = tr.push(x, feat, rcam, None)
        assert np.all(tr.history_length() == min(k + 1, 2))
        if k >= 1:
            assert np.array_equal(_bits(out), _bits(prev + (x - prev) * F(0.5)))
        prev = out


# ---------------------------------------------------------------- 3. refusals that need no device
def test_defaults():
    assert pt.temporal_defaults() == dict(max_history=32, normal_min=F(0.9), plane_tol=F(0.02), flags=0)


def test_refusals_without_a_device():
    L = _lib.lib()
    err = C.c_int(0)
    tp = _lib.TemporalParams()
    L.pt_temporal_defaults(C.byref(tp))
    L.pt_temporal_defaults(None)

    def create(params, w=24, h=16, order=0):
        err.value = 0
        h_ = L.pt_temporal_create(None, None if params is None else C.byref(params), w, h, order, C.byref(err))
        assert not h_ and err.value == _lib.PT_E_INVALID
        return L.pt_last_error().decode()

    assert "null" in create(None)
    assert "null context" in create(tp)                     # a valid request: only the context is missing
    for field, bad, word in (("max_history", 0, "max_history"), ("max_history", -3, "max_history"),
                             ("normal_min", 1.5, "normal_min"), ("normal_min", -1.5, "normal_min"),
                             ("normal_min", float("nan"), "normal_min"), ("plane_tol", 0.0, "plane_tol"),
                             ("plane_tol", -1.0, "plane_tol"), ("plane_tol", float("inf"), "plane_tol"), ("flags", 1, "flags")):
        p = _lib.TemporalParams()
        L.pt_temporal_defaults(C.byref(p))
        setattr(p, field, bad)
        assert word in create(p), (field, bad)
    assert "size" in create(tp, 0, 16) and "size" in create(tp, 24, 70000)
    assert "pixel order" in create(tp, 24, 16, 2)
    assert "Morton" in create(tp, 24, 16, _lib.PT_ORDER_MORTON) and "Morton" in create(tp, 24, 24, _lib.PT_ORDER_MORTON)
    assert "null context" in create(tp, 32, 32, _lib.PT_ORDER_MORTON)
    # the calls on an object
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, 24, 16)
    buf = (C.c_float * 4)()
    assert L.pt_temporal_push(None, C.byref(cam), None, 0, buf, buf, buf, None) == _lib.PT_E_INVALID
    assert b"null" in L.pt_last_error()
    assert L.pt_temporal_push_device(None, C.byref(cam), None, 0, buf, buf, buf, None, None) == _lib.PT_E_INVALID
    assert L.pt_temporal_length(None, buf) == _lib.PT_E_INVALID
    assert L.pt_temporal_reset(None) == _lib.PT_E_INVALID
    assert L.pt_temporal_frames(None) == 0
    L.pt_temporal_destroy(None)
