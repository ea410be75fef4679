"""Sub-pixel jitter's host surface (include/pt/pt.h, PT_FLAG_JITTER / PT_FLAG_JITTER_TENT): pt_jitter_offset and
pt_camera_ray_jitter against the numpy restatement of their arithmetic (jitter_ref), what the restatement itself is
worth (it discriminates, and a jittered render is anti-aliased), the refusal of the tent bit alone and the flags' way
through the two file headers.  No device."""
import ctypes as C
import struct

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
from cudapathtracer_amd import jitter_offset                 # (the parent has no such name: every test here errors there)
import jitter_ref
import oracle
import session_ref
import view_ref

F = np.float32
W, H, BOUNCES, SEED = 24, 16, 3, 1234
POS = (0.0, 1.0, 3.0)
GENERIC = view_ref.generic(POS)
BOX, TENT = pt.PT_FLAG_JITTER, pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT
# the smallest curand_uniform, the floats around 0.5 (the tent's two branches meet there), and the largest
EDGES = [F(2.0 ** -33), np.nextafter(F(0.5), F(0)), F(0.5), np.nextafter(F(0.5), F(1)), F(1.0)]
PIXELS = [(0, 0), (W - 1, H - 1), (65535, 0)]


def _view(v):
    return None if v is None else pt.make_view(v[0], v[1], v[2], v[3])


def _lib_ray(cam, view, px, py, jx, jy, lens, u1, u2):
    o, d = _lib.Vec3(), _lib.Vec3()
    _lib.lib().pt_camera_ray_jitter(C.byref(cam), None if view is None else C.byref(view), view_ref.morton(px, py), float(jx),
                                    float(jy), int(lens), float(u1), float(u2), C.byref(o), C.byref(d))
    return np.array((o.x, o.y, o.z), dtype=F), np.array((d.x, d.y, d.z), dtype=F)


def _stream(n):
    return oracle.uniform_stream(SEED, 77, n)


def test_jitter_offset_equals_the_restatement():
    assert jitter_ref.BOX_FLAGS == BOX and jitter_ref.TENT_FLAGS == TENT
    s = _stream(2000)
    pairs = [(a, b) for a in EDGES for b in EDGES] + list(zip(s[0::2], s[1::2]))
    assert len(pairs) == 25 + 1000
    for flags in (0, BOX, TENT, BOX | pt.PT_FLAG_NO_PRIMARY_CACHE, TENT | pt.PT_FLAG_COUNT):
        for ua, ub in pairs:
            got = np.array(jitter_offset(flags, ua, ub), dtype=F)
            want = np.array(jitter_ref.offset(flags, ua, ub), dtype=F)
            assert jitter_ref.same_bits(got, want) == 0, (flags, ua, ub, got, want)
    # the tent's range: the footprint's centre +- 1 pixel, centre at u = 0.5, both branches monotone
    lo, hi = jitter_offset(TENT, EDGES[0], EDGES[-1])
    assert -0.5 < lo < -0.4999 and hi == 1.5
    assert jitter_offset(TENT, 0.5, 0.5) == (0.5, 0.5)
    t = [jitter_offset(TENT, u, u)[0] for u in np.sort(s[:400])]
    assert all(a <= b for a, b in zip(t, t[1:]))
    assert jitter_offset(0, 0.3, 0.7) == (0.0, 0.0)


@pytest.mark.parametrize("view", [None, GENERIC], ids=["null_view", "generic"])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_camera_ray_jitter_equals_the_restatement(view, radius):
    cam = pt.make_camera(POS, 1.0, 3.0, radius, W, H)
    rcam = (POS, 1.0, 3.0, radius, W, H)
    v = _view(view)
    s = _stream(4000)
    cases = [(px, py, flags, ua, ub, 0.25, 0.75) for (px, py) in PIXELS for flags in (BOX, TENT) for ua in EDGES for ub in EDGES]
    for k in range(1000):   # stream values: the offset draws, then the lens pair, pixel and kind in rotation
        px, py = PIXELS[k % 3]
        cases.append((px, py, (BOX, TENT)[(k // 3) % 2], s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]))
    for px, py, flags, ua, ub, u1, u2 in cases:
        jx, jy = jitter_offset(flags, ua, ub)
        rjx, rjy = jitter_ref.offset(flags, ua, ub)
        for lens in (False, True):   # lens on with radius 0 is pixel 0's quirk; with a radius every pixel's
            o, d = _lib_ray(cam, v, px, py, jx, jy, lens, u1, u2)
            ro, rd = jitter_ref.ray(rcam, view, px, py, rjx, rjy, lens, u1, u2)
            assert jitter_ref.same_bits(o, ro) == 0 and jitter_ref.same_bits(d, rd) == 0, (px, py, flags, ua, ub, lens)
    # the public wrapper goes the same way
    o, d = _lib_ray(cam, v, 5, 3, 0.25, 0.625, False, 0, 0)
    got = pt.camera_ray(cam, view_ref.morton(5, 3), view=v, jitter=(0.25, 0.625))
    assert got == (tuple(float(c) for c in o), tuple(float(c) for c in d))


@pytest.mark.parametrize("view", [None, GENERIC], ids=["null_view", "generic"])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_zero_offsets_are_the_unjittered_ray(view, radius):
    """jx = jy = 0 is pt_camera_ray_view in every bit -- with a NULL view (pt_camera_ray) the signs of zeros too."""
    L = _lib.lib()
    cam = pt.make_camera(POS, 1.0, 3.0, radius, W, H)
    v = _view(view)
    vp = None if v is None else C.byref(v)
    s = _stream(2 * W * H)
    o, d = _lib.Vec3(), _lib.Vec3()
    signs = 0
    for y in range(H):
        for x in range(W):
            k = y * W + x
            for lens in (False, True):
                L.pt_camera_ray_view(C.byref(cam), vp, view_ref.morton(x, y), int(lens), float(s[2 * k]), float(s[2 * k + 1]),
                                     C.byref(o), C.byref(d))
                want = np.array((o.x, o.y, o.z, d.x, d.y, d.z), dtype=F)
                go, gd = _lib_ray(cam, v, x, y, 0.0, 0.0, lens, s[2 * k], s[2 * k + 1])
                assert jitter_ref.same_bits(np.concatenate([go, gd]), want) == 0, (x, y, lens)
                signs += int(np.count_nonzero(np.signbit(want) & (want == 0)))
    if view is None:
        assert signs > 0          # (negative zeros do occur: the comparison above covers them)


# ---- what the restatement is worth
@pytest.fixture(scope="module")
def osc():
    return oracle.OracleScene(load_scene("cornell").arrays())


def _differing_pixels(a, b):
    return int(np.count_nonzero(np.any(np.asarray(a) != np.asarray(b), axis=2)))


@pytest.mark.parametrize("integrator", [0, 1])
def test_the_restatement_discriminates(osc, integrator):
    """At 4 spp the box image differs from the unjittered one, from the tent one and from the one with ua and ub
    swapped in more than half of the frame's pixels (measured on integrator 0: 345, 307 and 305 of 384)."""
    rcam = (POS, 1.0, 3.0, 0.0, W, H)
    box = jitter_ref.render_cached("cornell", osc, rcam, None, BOX, 4, BOUNCES, integrator, SEED)
    plain = jitter_ref.render_cached("cornell", osc, rcam, None, 0, 4, BOUNCES, integrator, SEED)
    tent = jitter_ref.render_cached("cornell", osc, rcam, None, TENT, 4, BOUNCES, integrator, SEED)
    swapped = jitter_ref.render_cached("cornell", osc, rcam, None, BOX, 4, BOUNCES, integrator, SEED, swap=True)
    n = (_differing_pixels(box, plain), _differing_pixels(box, tent), _differing_pixels(box, swapped))
    print("integrator %d: box differs from plain / tent / swapped in %d / %d / %d of %d pixels" % ((integrator,) + n + (W * H,)))
    assert all(k > W * H // 2 for k in n), n
    # flags 0 is today's render: the oracle's own
    want, _ = oracle.render(osc, oracle.camera(POS, 1.0, 3.0, 0.0, W, H), W, H, 4, BOUNCES, integrator, SEED)
    assert jitter_ref.same_bits(np.asarray(plain), want) == 0


def test_jitter_anti_aliases(osc):
    """Cornell box, 24 x 16, 64 spp, integrator 0.  The truth is a 192 x 128 unjittered oracle render box-averaged 8 x 8:
    its 64 sub-pixel corners tile each coarse pixel's footprint.  The box-jittered image must be less than half as far
    from it (RMSE) as the unjittered one (measured: 0.145 against 1.04)."""
    spp, k = 64, 8
    fine, _ = oracle.render(osc, oracle.camera(POS, 1.0, 3.0, 0.0, W * k, H * k), W * k, H * k, spp, BOUNCES, 0, SEED)
    truth = fine.reshape(H, k, W, k, 3).mean(axis=(1, 3))
    plain, _ = oracle.render(osc, oracle.camera(POS, 1.0, 3.0, 0.0, W, H), W, H, spp, BOUNCES, 0, SEED)
    box = jitter_ref.render(osc, (POS, 1.0, 3.0, 0.0, W, H), None, BOX, spp, BOUNCES, 0, SEED)
    rmse = lambda a: float(np.sqrt(np.mean((np.asarray(a) - truth) ** 2)))   # noqa: E731
    e_plain, e_box = rmse(plain), rmse(box)
    print("RMSE against the box-averaged 192 x 128 render: unjittered %.4f, box-jittered %.4f" % (e_plain, e_box))
    assert e_box < 0.5 * e_plain, (e_box, e_plain)


# ---- refusals and the flags' way through the file headers
def test_tent_alone_is_refused():
    L = _lib.lib()
    jx, jy = C.c_float(7.0), C.c_float(7.0)
    assert L.pt_jitter_offset(pt.PT_FLAG_JITTER_TENT, 0.25, 0.75, C.byref(jx), C.byref(jy)) == pt.PT_E_INVALID
    assert b"PT_FLAG_JITTER_TENT" in L.pt_last_error()
    assert (jx.value, jy.value) == (7.0, 7.0)                      # a refused call changes nothing
    with pytest.raises(pt.PtError) as e:
        jitter_offset(pt.PT_FLAG_JITTER_TENT | pt.PT_FLAG_NO_PRIMARY_CACHE, 0.1, 0.2)
    assert e.value.code == pt.PT_E_INVALID and "PT_FLAG_JITTER_TENT" in str(e.value)
    assert L.pt_jitter_offset(BOX, 0.25, 0.75, None, C.byref(jy)) == pt.PT_E_INVALID
    assert (pt.PT_FLAG_JITTER, pt.PT_FLAG_JITTER_TENT) == (0x40, 0x80)
    assert L.pt_abi_version() == 6


@pytest.mark.parametrize("flags", [BOX, TENT, TENT | pt.PT_FLAG_NO_DEAD_PATH_SKIP])
def test_file_headers_carry_the_flags(tmp_path, flags):
    w, h = 6, 5
    # a checkpoint (format 1), packed by hand as pt.h documents it
    params = struct.pack("<6iQ5i4x", w, h, 0, 3, 0, flags, SEED, 0, 1, 0, 0, 0)
    cam = struct.pack("<6f2i", 0.0, 1.0, 3.0, 1.0, 3.0, 0.0, w, h)
    blob = struct.pack("<8sII", b"PTACCUM\0", 1, 128) + params + cam + struct.pack("<qQII", 4, 0x1234, 12, 0)
    assert len(blob) == 128
    f = tmp_path / "c.ptacc"
    f.write_bytes(blob + bytes(w * h * 48))
    info = pt.accum_file_info(str(f))
    assert info["params"].flags == flags and info["samples"] == 4
    # a session file (format 2)
    hd = session_ref.header(w, h, samples=4)
    hd["params"]["flags"] = flags
    g = str(tmp_path / "s.ptses")
    session_ref.write(g, hd)
    assert pt.session_file_info(g)["params"].flags == flags
