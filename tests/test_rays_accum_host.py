"""Accumulators and feature buffers over caller-supplied rays without a device (include/pt/pt.h, pt_accum_create_rays*,
pt_render_features_rays*): that the cases of tests/test_gpu_rays_accum.py and tests/test_gpu_rays_features.py
discriminate, the condition of their adaptive case, and the entry points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib

import adaptive_ref
import denoise_ref
import oracle
import rays_accum_ref as rar
import rays_ref

F = np.float32
W, H, BOUNCES, SEED = rar.W, rar.H, rar.BOUNCES, rar.SEED
POS = rays_ref.POS


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def osc(scene):
    return oracle.OracleScene(scene.arrays())


@pytest.mark.parametrize("integrator", [0, 1])
def test_means_differ_between_counts_and_from_the_lens_pixel(osc, integrator):
    """add(1), add(1), add(2) is checked against the restatement at 1, 2 and 4 samples: those three differ, and at
    Morton index 0 the restatement differs from the camera's render, which draws the quirk lens pair there.  (dist 3:
    with dist 1 pixel (0, 0) looks past the box and is black with either stream.)"""
    o, d = rays_ref.set_camera(pt, W, H, 3.0)
    m = rar.means(osc, "a3", o, d, integrator)
    m1, m2, m4 = m(1), m(2), m(4)
    for a, b in ((m1, m2), (m2, m4), (m1, m4)):
        assert np.any(a != b, axis=2).sum() > W * H // 4
    cam = oracle.camera(POS, 3.0, 3.0, 0.0, W, H)
    for n, mine in ((2, m2), (4, m4)):
        lens = oracle.render(osc, cam, W, H, n, BOUNCES, integrator, SEED, pixels=[0])[0]
        assert rays_ref.same_bits(lens[0, 0], mine[0, 0]) > 0, n


@pytest.mark.parametrize("name", ["b", "c"])
def test_ray_features_differ_from_the_camera_features(scene, osc, name):
    o, d = {"b": rays_ref.set_ortho, "c": rays_ref.set_panorama}[name](W, H)
    trace = lambda oo, dd: oracle.trace_batch(osc, oo, dd)                     # noqa: E731
    got = rar.features_ref(scene.arrays(), o, d, W, H, trace)
    cam = pt.make_camera(POS, 1.0, 3.0, 0.0, W, H)
    camf = denoise_ref.features_ref(scene.arrays(), cam, W, H, trace)
    differ = sum(got[y, x].tobytes() != camf[y, x].tobytes() for y in range(H) for x in range(W))
    print("set %s: %d of %d records differ from the camera's" % (name, differ, W * H))
    assert differ > W * H // 2
    assert (got["prim"] >= 0).sum() > W * H // 2                               # (the set sees the scene)
    # over the camera's own rays the two restatements are the same
    oc, dc = rays_ref.set_camera(pt, W, H)
    assert rar.features_ref(scene.arrays(), oc, dc, W, H, trace).tobytes() == camf.tobytes()


@pytest.mark.parametrize("integrator", [0, 1])
def test_adaptive_case_condition(osc, integrator):
    """The loop case of the GPU test -- the panorama set, passes of 4, cap 32, tol 0.2 (the project's cornell_blob
    values) -- freezes some pixels but not all, at two or more distinct counts.  A condition on the input, from the
    restatement.  tol 0.2 gives it: integrator 0 freezes 282 of 384 pixels, integrator 1 313 of 384, both at every
    count from 8 to 32 in steps of 4."""
    o, d = rays_ref.set_panorama(W, H)
    sim = adaptive_ref.simulate(rar.means(osc, "c", o, d, integrator), (H, W), **rar.LOOP)
    counts = sim["counts"]
    frozen = W * H - sim["active"]
    at = sorted(int(v) for v in np.unique(counts))
    print("integrator %d: frozen %d of %d, counts %s, passes %d, samples_total %d" % (integrator, frozen, W * H, at, sim["passes"],
                                                                                      sim["samples_total"]))
    assert 0 < frozen < W * H
    early = sorted(set(at) - {rar.LOOP["cap"]})                                # counts below the cap are frozen-at counts
    assert len(early) >= 2, at


def test_entry_points_refuse_null_arguments():
    L = _lib.lib()
    p = pt.Renderer.params(8, 8, 0)
    b = (C.c_float * 8)()
    err = C.c_int(0)
    assert not L.pt_accum_create_rays(None, C.byref(p), b, C.byref(err)) and err.value == pt.PT_E_INVALID
    err = C.c_int(0)
    assert not L.pt_accum_create_rays_device(None, C.byref(p), b, None, C.byref(err)) and err.value == pt.PT_E_INVALID
    assert b"pt_accum_create_rays" in L.pt_last_error()
    assert L.pt_accum_has_rays(None) == 0
    assert L.pt_render_features_rays(None, C.byref(p), b, b) == pt.PT_E_INVALID
    assert L.pt_render_features_rays_device(None, C.byref(p), b, b, None) == pt.PT_E_INVALID
    assert b"pt_render_features_rays" in L.pt_last_error()
