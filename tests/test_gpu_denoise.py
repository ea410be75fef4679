"""The preview denoiser on the GPU (pt_denoise*): every case is compared bit for bit with the numpy
restatement of the header's arithmetic (tests/denoise_ref.py), on the default kernel (taps staged through
LDS) and on the direct-gather instantiation (PT_DENOISE_DIRECT=1), which must also equal each other."""
import contextlib
import os

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import scenes

import denoise_ref

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def direct_gather(on, tiled_max=None):
    """The library reads its knobs at every call: PT_DENOISE_DIRECT=1 runs every iteration on the direct gather,
    PT_DENOISE_TILED_MAX moves the largest LDS-staged step (default 4, at most 16)."""
    old = {k: os.environ.pop(k, None) for k in ("PT_DENOISE_DIRECT", "PT_DENOISE_TILED_MAX")}
    if on:
        os.environ["PT_DENOISE_DIRECT"] = "1"
    if tiled_max is not None:
        os.environ["PT_DENOISE_TILED_MAX"] = str(tiled_max)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def both_kernels(r, img, feat, **kw):
    """The filtered image, after checking that the tiled and the direct-gather kernels agree in every bit."""
    with direct_gather(False):
        tiled = r.denoise(img, feat, **kw)
    with direct_gather(True):
        direct = r.denoise(img, feat, **kw)
    assert tiled.tobytes() == direct.tobytes(), "tiled and direct-gather kernels differ"
    with direct_gather(False, tiled_max=16):   # the LDS-staged kernel at steps 8 and 16 too (not the default there)
        staged16 = r.denoise(img, feat, **kw)
    assert staged16.tobytes() == direct.tobytes(), "LDS staging at steps 8 / 16 differs from the direct gather"
    return tiled


def check(r, img, feat, **kw):
    got = both_kernels(r, img, feat, **kw)
    ref = denoise_ref.denoise_ref(img, feat, **kw)
    bad = int(np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32)))
    assert bad == 0, "%d of %d values differ from the numpy reference" % (bad, got.size)
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    assert got[skip].tobytes() == np.ascontiguousarray(img, dtype=np.float32)[skip].tobytes()
    return got


@pytest.fixture(scope="module")
def blob():
    s = load_scene("cornell_blob")
    cache = {}
    with pt.Renderer(s, 0) as r:
        def inputs(w, h):
            if (w, h) not in cache:
                cam = pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)
                cache[(w, h)] = (r.render(cam, w, h, 4, bounces=3, seed=1234)[0], r.features(cam, w, h))
            return cache[(w, h)]
        yield r, inputs


@pytest.mark.parametrize("w,h", [(24, 16), (37, 19), (70, 50), (130, 70)])
def test_sizes_five_iterations(blob, w, h):
    """24x16: steps 8 and 16 reach outside the image on every side; 70x50 and 130x70 cross the 64-pixel tile and
    the lattice-row tiles in both directions."""
    r, inputs = blob
    img, feat = inputs(w, h)
    assert (feat["prim"] < 0).any() and (feat["prim"] >= 0).any()
    out = check(r, img, feat)
    assert out.tobytes() != img.tobytes()


@pytest.mark.parametrize("iterations", [0, 1, 5, 8])
def test_iterations(blob, iterations):
    r, inputs = blob
    img, feat = inputs(37, 19)
    out = check(r, img, feat, iterations=iterations)
    if iterations == 0:
        assert out.tobytes() == img.tobytes()


@pytest.mark.parametrize("kw", [dict(sigma_color=2.0), dict(demodulate=False), dict(normal_power_log2=0),
                                dict(normal_power_log2=7), dict(sigma_color=0.5, demodulate=False, iterations=3)],
                         ids=["sigma_color", "no_demodulate", "npow0", "npow7", "mixed"])
def test_parameters(blob, kw):
    r, inputs = blob
    img, feat = inputs(70, 50)
    check(r, img, feat, **kw)


def test_in_place_and_device_pointers(blob):
    import torch
    r, inputs = blob
    w, h = 70, 50
    img, feat = inputs(w, h)
    ref = denoise_ref.denoise_ref(img, feat)
    d_feat = torch.from_numpy(np.frombuffer(feat.tobytes(), dtype=np.uint8).copy()).cuda()
    for direct in (False, True):
        d_img = torch.from_numpy(img.copy()).cuda()
        d_out = torch.zeros_like(d_img)
        with direct_gather(direct):
            r.denoise_device(d_img.data_ptr(), d_feat.data_ptr(), d_out.data_ptr(), w, h)
            r.denoise_device(d_img.data_ptr(), d_feat.data_ptr(), d_img.data_ptr(), w, h)      # d_out == d_in
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == ref.tobytes()
        assert d_img.cpu().numpy().tobytes() == ref.tobytes()


def test_morton_order(blob):
    r, inputs = blob
    w = h = 32
    img, feat = inputs(w, h)
    idx = np.array([[pt.morton_pxl_to_i(x, y) for x in range(w)] for y in range(h)])
    mimg = np.zeros((w * h, 3), dtype=np.float32)
    mfeat = np.zeros(w * h, dtype=pt.FEATURE)
    mimg[idx] = img
    mfeat[idx] = feat
    cam = pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)
    assert r.features(cam, w, h, pixel_order=1).tobytes() == mfeat.tobytes()
    ref = denoise_ref.denoise_ref(img, feat)
    got = both_kernels(r, mimg, mfeat, pixel_order=1)
    assert got[idx].tobytes() == ref.tobytes()


def _synthetic(w, h, seed, all_skip=False):
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w), dtype=pt.FEATURE)
    n = rng.normal(size=(h, w, 3))
    unit = n / np.linalg.norm(n, axis=2)[..., None]
    f["normal"] = np.where(rng.random((h, w, 1)) < 0.5, unit, unit * rng.uniform(0.3, 1.5, (h, w, 1)))   # unit and not
    # (lengths <= 1.5: the normal weight, a 32nd power by default, stays finite)
    f["normal"][rng.random((h, w)) < 0.3] = f["normal"][0, 0]                                          # and equal ones
    f["position"] = rng.uniform(-5, 5, (h, w, 3))
    f["position"][:, : w // 2] *= 0.01                                                                 # nearly coplanar
    f["depth"] = rng.uniform(0.1, 50, (h, w))
    f["albedo"] = rng.uniform(0, 1, (h, w, 3))
    f["albedo"][rng.random((h, w)) < 0.1] = 0.0                                                        # below 1e-3
    f["prim"] = rng.integers(0, 1000, (h, w))
    kind = rng.random((h, w))
    f["prim"][kind < 0.1] = -1
    f["prim"][(kind >= 0.1) & (kind < 0.2)] |= pt.PT_FEATURE_EMISSIVE
    f["prim"][5] = -1                               # whole pass-through rows
    f["prim"][h - 1] |= pt.PT_FEATURE_EMISSIVE
    if all_skip:
        f["prim"] = -1
    img = rng.uniform(0, 10, (h, w, 3)).astype(np.float32)
    return img, f


@pytest.mark.parametrize("kw", [dict(), dict(sigma_color=2.0), dict(normal_power_log2=0, demodulate=False),
                                dict(iterations=8, sigma_depth=5.0)], ids=["default", "sigma_color", "npow0_raw", "wide"])
def test_synthetic_features(blob, kw):
    """Weights Cornell never produces: random unit and non-unit normals, random positions, depths in
    [0.1, 50], about 20% pass-through pixels with whole pass-through rows, colours in [0, 10]."""
    r, _ = blob
    img, feat = _synthetic(45, 33, 7)
    out = check(r, img, feat, **kw)
    assert np.isfinite(out).all()


def test_all_pass_through(blob):
    r, _ = blob
    img, feat = _synthetic(45, 33, 8, all_skip=True)
    assert check(r, img, feat).tobytes() == img.tobytes()


def test_parameter_refusals(blob):
    r, inputs = blob
    img, feat = inputs(24, 16)
    bad = [dict(iterations=9), dict(iterations=-1), dict(normal_power_log2=8), dict(sigma_depth=0.0),
           dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_depth=-1.0)]
    for kw in bad:
        with pytest.raises(pt.PtError) as e:
            r.denoise(img, feat, **kw)
        assert e.value.code == pt.PT_E_INVALID, kw
    import ctypes as C
    from cudapathtracer_amd import _lib
    dp = pt.Renderer.denoise_params()
    dp.flags = 0x2                                  # an unknown flag
    out = np.empty_like(img)
    L = _lib.lib()
    assert L.pt_denoise(r._h, C.byref(dp), 24, 16, 0, img.ctypes.data, feat.ctypes.data, out.ctypes.data) == pt.PT_E_INVALID
    dp.flags = 0
    assert L.pt_denoise(r._h, C.byref(dp), 24, 16, 1, img.ctypes.data, feat.ctypes.data, out.ctypes.data) == pt.PT_E_INVALID
    assert b"Morton" in L.pt_last_error()
    assert L.pt_denoise(r._h, C.byref(dp), 0, 16, 0, img.ctypes.data, feat.ctypes.data, out.ctypes.data) == pt.PT_E_INVALID
    assert L.pt_denoise(r._h, C.byref(dp), 24, 16, 0, None, feat.ctypes.data, out.ctypes.data) == pt.PT_E_INVALID


def test_refused_while_a_render_is_in_flight(blob):
    import torch
    r, inputs = blob
    w, h = 24, 16
    img, feat = inputs(w, h)
    cam = pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)
    d = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    r.render_device_async(cam, d.data_ptr(), w, h, 2)
    try:
        with pytest.raises(pt.PtError) as e:
            r.denoise(img, feat)
        assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
        with pytest.raises(pt.PtError) as e:
            r.features(cam, w, h)
        assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
    finally:
        r.wait()
    check(r, img, feat)


def test_quality_on_the_gpu_output(blob):
    """The host test's condition on the GPU's own output: the filtered 64x64 / 4-spp / seed-1234 render is at most
    0.5x as far (RMSE) from the oracle's 2048-spp seed-99 render as the noisy one."""
    import oracle
    r, inputs = blob
    w = h = 64
    img, feat = inputs(w, h)
    kw = scenes.CORNELL_CAMERA
    osc = oracle.OracleScene(load_scene("cornell_blob").arrays())
    ocam = oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], kw["radius"], w, h)
    clean = oracle.render(osc, ocam, w, h, 2048, 3, 0, 99)[0].astype(np.float32)
    out = check(r, img, feat)
    e_noisy, e_out = denoise_ref.rmse(img, clean), denoise_ref.rmse(out, clean)
    print("rmse noisy %.4f filtered %.4f ratio %.3f" % (e_noisy, e_out, e_out / e_noisy))
    assert e_out <= 0.5 * e_noisy


def test_accumulator_preview(blob):
    r, inputs = blob
    w, h = 37, 19
    img, feat = inputs(w, h)
    cam = pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)
    with r.accumulator(cam, w, h, bounces=3, seed=1234) as acc:
        acc.add(2)
        acc.add(2)
        preview = r.denoise(acc.image(), feat)
    assert preview.tobytes() == r.denoise(img, feat).tobytes()
