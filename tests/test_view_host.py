"""The oriented camera's host surface (include/pt/pt.h, pt_view): pt_camera_ray_view against the numpy restatement of
its arithmetic (view_ref), the look-at and field-of-view helpers, the view's validation, format version 3 of the
session header, and pt_cli's argument errors.  No device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
import session_ref
import view_ref

F = np.float32
CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
POS = (0.0, 1.0, 3.0)
VIEWS = {
    "yaw90": view_ref.YAW90,
    "generic": view_ref.generic(POS),
    "mirror": view_ref.MIRROR,
    "film": view_ref.with_film(view_ref.generic(POS), (1.5, 1.0)),
    "identity": view_ref.IDENTITY,
}


def _view(v):
    return pt.make_view(v[0], v[1], v[2], v[3])


def _lib_rays(cam, view, idxs, lens, u1, u2):
    L = _lib.lib()
    o, d = _lib.Vec3(), _lib.Vec3()
    out_o, out_d = np.empty((len(idxs), 3), dtype=F), np.empty((len(idxs), 3), dtype=F)
    vp = None if view is None else C.byref(view)
    for i, idx in enumerate(idxs):
        L.pt_camera_ray_view(C.byref(cam), vp, int(idx), int(lens), float(u1[i]), float(u2[i]), C.byref(o), C.byref(d))
        out_o[i] = (o.x, o.y, o.z)
        out_d[i] = (d.x, d.y, d.z)
    return out_o, out_d


@pytest.mark.parametrize("size", [(24, 16), (37, 19)])
@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("name", sorted(VIEWS))
def test_camera_ray_view_equals_the_restatement(name, radius, size):
    """Every pixel, bit for bit; with a lens, random draws; pixel index 0 is among the pixels, with and without
    lens draws (it is a lens unit even for radius 0)."""
    W, H = size
    v = VIEWS[name]
    cam = pt.make_camera(POS, 1.0, 3.0, radius, W, H)
    rcam = (POS, 1.0, 3.0, radius, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    idxs = [view_ref.morton(int(x), int(y)) for x, y in zip(xs, ys)]
    assert idxs[0] == 0
    rng = np.random.default_rng(7 + W)
    u1 = rng.random(len(xs), dtype=F)
    u2 = rng.random(len(xs), dtype=F)
    for lens in ((False, True) if radius else (False,)):
        o, d = _lib_rays(cam, _view(v), idxs, lens, u1, u2)
        ro, rd = view_ref.rays(rcam, v, xs, ys, lens, u1, u2)
        assert view_ref.same_bits(o, ro) == 0 and view_ref.same_bits(d, rd) == 0, (name, lens)
        if not lens:
            assert np.all(o == np.asarray(POS, dtype=F))
    # pixel 0 with the lens draws of a radius-0 camera (the reference's quirk pixel)
    o, d = _lib_rays(cam, _view(v), [0], True, u1[:1], u2[:1])
    ro, rd = view_ref.rays(rcam, v, [0], [0], True, u1[:1], u2[:1])
    assert view_ref.same_bits(o, ro) == 0 and view_ref.same_bits(d, rd) == 0
    # the public wrapper goes the same way
    o, d = _lib_rays(cam, _view(v), [idxs[5]], False, [0], [0])
    assert pt.camera_ray(cam, idxs[5], view=_view(v)) == (tuple(float(c) for c in o[0]), tuple(float(c) for c in d[0]))


def test_yaw_view_has_exact_zeros_and_differs_from_the_null_view():
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, 24, 16)
    o, d = _lib_rays(cam, _view(view_ref.YAW90), [view_ref.morton(12, 8)], False, [0], [0])
    # the centre pixel: camera-space (0, 0, -3) -> world -3 * back = (-3, 0, 0)
    assert tuple(d[0]) == (-1.0, 0.0, 0.0)
    o0, d0 = _lib_rays(cam, None, [view_ref.morton(12, 8)], False, [0], [0])
    assert tuple(d0[0]) == (0.0, 0.0, -1.0)


@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_null_view_is_pt_camera_ray(radius):
    W, H = 24, 16
    cam = pt.make_camera(POS, 1.0, 3.0, radius, W, H)
    rng = np.random.default_rng(3)
    for lens in (0, 1):
        for idx in range(0, 600, 7):
            u1, u2 = float(rng.random(dtype=F)), float(rng.random(dtype=F))
            a = pt.camera_ray(cam, idx, lens, u1, u2)
            o, d = _lib_rays(cam, None, [idx], lens, [u1], [u2])
            assert view_ref.same_bits(np.asarray(a[0], dtype=F), o[0]) == 0
            assert view_ref.same_bits(np.asarray(a[1], dtype=F), d[0]) == 0


def test_look_at():
    v = pt.look_at(POS, (0, 1, 0), (0, 1, 0))   # the reference camera's pose
    assert (tuple(v.right), tuple(v.up), tuple(v.back), v.film_w, v.film_h) == ((1, 0, 0), (0, 1, 0), (0, 0, 1), 1, 1)
    rng = np.random.default_rng(11)
    for _ in range(200):
        pos, tgt, up = (rng.normal(size=3).astype(F) * F(3) for _ in range(3))
        v = pt.look_at(pos, tgt, up)
        r, u, b = view_ref.look_at64(pos, tgt, up)
        for got, want in ((v.right, r), (v.up, u), (v.back, b)):
            assert view_ref.same_bits(np.array(list(got), dtype=F), want) == 0
        assert (v.film_w, v.film_h) == (1.0, 1.0)
        assert _lib.lib().pt_view_validate(C.byref(v)) == 0          # the result passes its own validation
    for pos, tgt, up, word in (((1, 2, 3), (1, 2, 3), (0, 1, 0), "target"),         # pos == target
                               ((0, 0, 0), (0, 5, 0), (0, 1, 0), "parallel"),       # up parallel to back
                               ((0, 0, 0), (0, -5, 0), (0, 2, 0), "parallel"),      # ... antiparallel
                               ((1, 2, 3), (0, 0, 0), (2, 4, 6), "parallel"),       # ... a generic parallel pair
                               ((0, 0, 0), (0, 0, 1), (0, 0, 0), "parallel"),       # a zero up
                               ((float("nan"), 0, 0), (0, 0, 1), (0, 1, 0), "finite"),
                               ((0, 0, 0), (float("inf"), 0, 1), (0, 1, 0), "finite"),
                               ((0, 0, 0), (0, 0, 1), (0, float("nan"), 0), "finite")):
        with pytest.raises(pt.PtError) as e:
            pt.look_at(pos, tgt, up)
        assert e.value.code == pt.PT_E_INVALID and word in str(e.value), str(e.value)
    assert _lib.lib().pt_view_look_at(_lib.Vec3(0, 0, 1), _lib.Vec3(0, 0, 0), _lib.Vec3(0, 1, 0), None) == pt.PT_E_INVALID


def _adjacent(a, b):
    a, b = F(a), F(b)
    return a == b or np.nextafter(a, b) == b


def test_set_fov():
    L = _lib.lib()
    for dist, vfov, W, H in ((1.0, 60.0, 1920, 1080), (1.0, 90.0, 24, 16), (0.7, 35.5, 37, 19), (2.5, 179.0, 16, 16),
                             (1.0, 0.5, 640, 480)):
        cam = pt.make_camera(POS, dist, 3.0, 0.0, W, H)
        v = pt.look_at(POS, (0.3, 0.7, -0.2), vfov=vfov, cam=cam)
        want_h = 2.0 * float(F(dist)) * math.tan(math.radians(float(F(vfov))) / 2.0)
        assert _adjacent(v.film_h, want_h), (v.film_h, want_h)
        # square pixels: film_w / film_h == W / H to 1 ulp.  Both are rounded once from doubles whose quotient is W / H
        # to double rounding, so each is off by at most 2^-24 relative and their quotient by (1 + 2^-24) / (1 - 2^-24) - 1
        ratio = float(v.film_w) / float(v.film_h)
        assert abs(ratio / (W / H) - 1.0) <= 2.0 ** -23 * (1.0 + 2.0 ** -23), (ratio, W / H)
        # the basis is the look-at's
        b = pt.look_at(POS, (0.3, 0.7, -0.2))
        assert (tuple(v.right), tuple(v.up), tuple(v.back)) == (tuple(b.right), tuple(b.up), tuple(b.back))
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, 24, 16)
    v = _view(view_ref.IDENTITY)
    for bad in (0.0, 180.0, -5.0, 200.0, float("nan")):
        assert L.pt_view_set_fov(C.byref(v), C.byref(cam), bad, 24, 16) == pt.PT_E_INVALID
        assert b"vfov" in L.pt_last_error()
    assert L.pt_view_set_fov(C.byref(v), C.byref(cam), 60.0, 0, 16) == pt.PT_E_INVALID
    assert L.pt_view_set_fov(C.byref(v), C.byref(cam), 60.0, 24, -1) == pt.PT_E_INVALID
    assert L.pt_view_set_fov(None, C.byref(cam), 60.0, 24, 16) == pt.PT_E_INVALID
    assert (v.film_w, v.film_h) == (1.0, 1.0)                       # a refused call changes nothing
    with pytest.raises(ValueError):
        pt.look_at(POS, (0, 0, 0), vfov=60.0)


def _bad_views():
    """(view, word of the message): each of the 6 orthonormality terms broken in turn, then the other refusals."""
    e = 2e-3
    r, u, b = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    yield ((1.0 + e, 0, 0), u, b, (1, 1)), "right.right"
    yield (r, (0, 1.0 - e, 0), b, (1, 1)), "up.up"
    yield (r, u, (0, 0, 1.0 + e), (1, 1)), "back.back"
    # a sheared pair stays unit length to 1e-6 (e^2/2) and breaks only its own dot product
    s = math.sqrt(1.0 - e * e)
    yield ((s, e, 0), u, b, (1, 1)), "right.up"
    yield ((s, 0, e), u, b, (1, 1)), "right.back"
    yield (r, (0, s, e), b, (1, 1)), "up.back"
    yield ((float("nan"), 0, 0), u, b, (1, 1)), "finite"
    yield (r, u, b, (float("inf"), 1)), "finite"
    yield (r, u, b, (0, 1)), "film"
    yield (r, u, b, (1, -1)), "film"
    yield ((0, 0, 0), u, b, (1, 1)), "right.right"


def test_view_validation():
    L = _lib.lib()
    for v in list(VIEWS.values()) + [((1 + 4e-4, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1)),           # r.r - 1 = 8e-4: inside
                                     ((1, 0, 0), (5e-4, 1, 0), (0, 0, 1), (3.5, 0.01))]:
        assert L.pt_view_validate(C.byref(_view(v))) == 0, v
    for v, word in _bad_views():
        assert L.pt_view_validate(C.byref(_view(v))) == pt.PT_E_INVALID, v
        assert word in L.pt_last_error().decode(), (word, L.pt_last_error())
    assert L.pt_view_validate(None) == pt.PT_E_INVALID
    # the render entry points validate before they touch a device: a null context still comes first
    assert L.pt_render_view(None, None, None, None, None, None) == pt.PT_E_INVALID


# ---- session header, format version 3: version 2's 192 bytes, the view at 192..235, zeros to 255
W, H = 6, 5
VIEW_REC = np.dtype([("right", "<f4", (3,)), ("up", "<f4", (3,)), ("back", "<f4", (3,)), ("film_w", "<f4"), ("film_h", "<f4")])
assert VIEW_REC.itemsize == 44


def _v3_file(path, view=VIEWS["film"], version=3, header_bytes=256, pad=bytes(20), cut=0, tail=True, **kw):
    h = session_ref.header(W, H, version=version, header_bytes=header_bytes, **kw)
    rec = np.zeros((), dtype=VIEW_REC)
    rec["right"], rec["up"], rec["back"], rec["film_w"], rec["film_h"] = view[0], view[1], view[2], view[3][0], view[3][1]
    blob = h.tobytes() + (rec.tobytes() + pad if tail else b"") + bytes(W * H * 48)
    if cut:
        blob = blob[:cut]
    with open(path, "wb") as f:
        f.write(blob)
    return rec


def _refused(path, fn=None):
    with pytest.raises(pt.PtError) as e:
        (fn or pt.session_file_info)(path)
    return e.value.code, str(e.value)


def test_session_header_version_3(tmp_path):
    f = str(tmp_path / "s.ptses")
    rec = _v3_file(f, samples=8)
    info = pt.session_file_info(f)
    assert info["samples"] == 8 and info["params"].width == W
    v = pt.session_file_view(f)
    got = np.zeros((), dtype=VIEW_REC)
    got["right"], got["up"], got["back"], got["film_w"], got["film_h"] = list(v.right), list(v.up), list(v.back), v.film_w, v.film_h
    assert got.tobytes() == rec.tobytes()
    for reader in (pt.session_file_info, pt.session_file_view):
        _v3_file(f, header_bytes=192, tail=False)                          # version 3 with version 2's header
        code, msg = _refused(f, reader)
        assert code == pt.PT_E_INVALID and "version 3" in msg and "header" in msg
        _v3_file(f, version=2)                                             # version 2 with version 3's header
        code, msg = _refused(f, reader)
        assert code == pt.PT_E_INVALID and "header" in msg
        for k in (0, 7, 19):                                               # a non-zero byte in 236..255
            pad = bytearray(20)
            pad[k] = 1
            _v3_file(f, pad=bytes(pad))
            code, msg = _refused(f, reader)
            assert code == pt.PT_E_INVALID and "236..255" in msg
        for bad, word in _bad_views():                                     # a stored view that is not valid
            _v3_file(f, view=bad)
            code, msg = _refused(f, reader)
            assert code == pt.PT_E_INVALID and word in msg, (bad, msg)
        for cut in (193, 210, 236, 255):                                   # truncation inside the view's part
            _v3_file(f, cut=cut)
            code, msg = _refused(f, reader)
            assert code == pt.PT_E_IO and "truncated" in msg, (cut, msg)
        _v3_file(f, cut=256 + W * H * 48 - 1)                              # ... and inside the sections, as before
        code, msg = _refused(f, reader)
        assert code == pt.PT_E_IO and "truncated" in msg
    # the format-1 reader names the version it met
    _v3_file(f)
    code, msg = _refused(f, pt.accum_file_info)
    assert code == pt.PT_E_INVALID and "format version 3, this build reads 1" in msg


def test_version_2_file_has_no_view(tmp_path):
    f = str(tmp_path / "s.ptses")
    session_ref.write(f, session_ref.header(W, H, samples=4))
    assert pt.session_file_view(f) is None
    has = C.c_int(7)
    assert _lib.lib().pt_session_file_view(f.encode(), None, C.byref(has)) == 0 and has.value == 0
    assert _lib.lib().pt_session_file_view(None, None, None) == pt.PT_E_INVALID


def test_accum_view_rejects_null():
    L = _lib.lib()
    assert L.pt_accum_view(None, None, None) == pt.PT_E_INVALID
    err = C.c_int(0)
    assert not L.pt_accum_create_view(None, None, None, None, C.byref(err)) and err.value == pt.PT_E_INVALID


# ---- pt_cli: argument errors (no device is reached)
def _cli(*args):
    obj = os.path.join(MODELS, "cornell.obj")
    return subprocess.run([CLI, "--obj", obj] + list(args), capture_output=True, text=True, timeout=120)


def test_cli_view_argument_errors():
    for bad in ("1,2", "a,b,c", "1,2,3,4", "1,2,3x"):
        r = _cli("--look-at", bad)
        assert r.returncode == 2 and "--look-at" in r.stderr, (bad, r.stderr)
    r = _cli("--look-at")
    assert r.returncode == 2 and "missing value" in r.stderr
    for bad in ("0", "180", "-3", "nan"):
        r = _cli("--look-at", "0,1,0", "--vfov", bad)
        assert r.returncode == 2 and "--vfov" in r.stderr, (bad, r.stderr)
    r = _cli("--cam", "0.5,1,2", "--look-at", "0.5,1,2")                   # the target is the position
    assert r.returncode == 1 and "--look-at" in r.stderr and "target" in r.stderr
    r = _cli("--look-at", "0,5,3", "--up", "0,1,0", "--cam", "0,1,3")      # up parallel to the viewing direction
    assert r.returncode == 1 and "parallel" in r.stderr
    r = _cli("--film", "1.5")
    assert r.returncode == 2 and "--film" in r.stderr
    r = _cli("--film", "0,1")
    assert r.returncode == 2 and "--film" in r.stderr
    r = _cli("--look-at", "0,1,0", "--vfov", "40", "--film", "1,1")
    assert r.returncode == 2 and "choose one" in r.stderr
