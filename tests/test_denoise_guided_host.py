"""The variance-guided denoiser without a GPU: the C-ABI's layout, defaults and refusals, and the numpy restatement
(tests/denoise_guided_ref.py) on the oracle's own renders -- with the variance unknown it is denoise_ref bit for bit,
and with NoiseRef's variance it removes noise at 4 samples and still improves the image at 128, where the plain
filter has started to make it worse."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, scenes

import denoise_guided_ref
import denoise_ref
import noise_ref

W = H = 64
SEED, BOUNCES = 1234, 3


def test_layout_and_defaults():
    assert C.sizeof(_lib.DenoiseGuidedParams) == 24
    assert _lib.DenoiseGuidedParams.base.offset == 0 and _lib.DenoiseGuidedParams.sigma_luma.offset == 20
    gp = _lib.DenoiseGuidedParams(_lib.DenoiseParams(-1, -1, -1.0, -1.0, 99), -1.0)
    _lib.lib().pt_denoise_guided_defaults(C.byref(gp))
    dp = _lib.DenoiseParams()
    _lib.lib().pt_denoise_defaults(C.byref(dp))
    assert bytes(gp.base) == bytes(dp) and gp.sigma_luma == 2.0
    _lib.lib().pt_denoise_guided_defaults(None)
    d = pt.denoise_guided_defaults()
    assert d["sigma_luma"] == 2.0 and {k: d[k] for k in pt.denoise_defaults()} == pt.denoise_defaults()


def test_null_and_sigma_luma_refusals():
    L = _lib.lib()
    gp = pt.Renderer.denoise_guided_params()
    buf = np.zeros(8 * 8 * 12, dtype=np.float32)
    b = buf.ctypes.data
    calls = [
        lambda: L.pt_denoise_guided(None, C.byref(gp), 8, 8, 0, b, b, b, b),               # no context
        lambda: L.pt_denoise_guided(None, C.byref(gp), 8, 8, 0, b, b, None, b),            # no variance
        lambda: L.pt_denoise_guided(None, None, 8, 8, 0, b, b, b, b),
        lambda: L.pt_denoise_guided_device(None, C.byref(gp), 8, 8, 0, b, b, b, b, None),
        lambda: L.pt_denoise_guided_device(None, C.byref(gp), 8, 8, 0, b, b, None, b, None),
        lambda: L.pt_denoise_guided_device(None, None, 8, 8, 0, None, None, None, None, None),
        lambda: L.pt_noise_variance(None, b),
        lambda: L.pt_noise_variance_device(None, b, None),
    ]
    for call in calls:
        assert call() == _lib.PT_E_INVALID
        assert b"null" in L.pt_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        gp = pt.Renderer.denoise_guided_params(sigma_luma=bad)
        assert L.pt_denoise_guided(None, C.byref(gp), 8, 8, 0, b, b, b, b) == _lib.PT_E_INVALID
        assert b"pt_denoise_guided: sigma_luma" in L.pt_last_error()
        assert L.pt_denoise_guided_device(None, C.byref(gp), 8, 8, 0, b, b, b, b, None) == _lib.PT_E_INVALID
        assert b"pt_denoise_guided_device: sigma_luma" in L.pt_last_error()


@pytest.fixture(scope="module")
def blob():
    """The oracle's cornell_blob 64x64: render(n) (f64 mean after n samples, seed 1234, integrator 0), the 2048-spp
    seed-99 render and the oracle-traced features."""
    import oracle
    arrays = load_scene("cornell_blob").arrays()
    osc = oracle.OracleScene(arrays)
    kw = scenes.CORNELL_CAMERA
    ocam = oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], kw["radius"], W, H)
    feat = denoise_ref.features_ref(arrays, pt.make_camera(width=W, height=H, **kw), W, H,
                                    lambda o, d: oracle.trace_batch(osc, o, d))
    clean = oracle.render(osc, ocam, W, H, 2048, BOUNCES, 0, 99)[0].astype(np.float32)
    return (lambda n: oracle.render(osc, ocam, W, H, n, BOUNCES, 0, SEED)[0]), clean, feat


def _progressive(render, passes, spp):
    """(fp32 mean image, variance map) after `passes` passes of `spp` samples, the variance from NoiseRef."""
    est = noise_ref.NoiseRef(0, shape=(H, W))
    for k in range(1, passes + 1):
        mean = render(k * spp)
        assert est.update(k * spp, mean)
    return mean.astype(np.float32), denoise_guided_ref.variance_ref(est, passes * spp)


@pytest.mark.parametrize("kw", [dict(), dict(sigma_color=0.5)], ids=["default", "sigma_color"])
def test_unknown_variance_is_the_plain_filter(blob, kw):
    """With var = +inf the luminance weight is exactly 1 on every tap: denoise_ref's output byte for byte."""
    render, _, feat = blob
    noisy = render(4).astype(np.float32)
    want = denoise_ref.denoise_ref(noisy, feat, **kw)
    assert want.tobytes() != noisy.tobytes()
    for unknown in (np.inf, np.nan, -1.0, 1e30):
        got = denoise_guided_ref.denoise_guided_ref(noisy, feat, np.full((H, W), unknown, dtype=np.float32), **kw)
        assert got.tobytes() == want.tobytes(), unknown


def test_variance_map_of_the_restatement(blob):
    """variance_ref is the window variance when the window starts at 0, +inf before two batches, and scales by W/n
    for an estimator attached late."""
    render, _, _ = blob
    est = noise_ref.NoiseRef(0, shape=(H, W))
    est.update(2, render(2))
    assert np.isposinf(denoise_guided_ref.variance_ref(est, 2)).all()
    est.update(4, render(4))
    v = denoise_guided_ref.variance_ref(est, 4)
    assert v.dtype == np.float32 and v.tobytes() == (est.m2 / (1.0 * est.W)).astype(np.float32).tobytes()
    late = noise_ref.NoiseRef(2, render(2))
    late.update(3, render(3))
    late.update(4, render(4))
    assert late.W == 2.0
    assert denoise_guided_ref.variance_ref(late, 4).tobytes() == (late.m2 / (1.0 * 4.0)).astype(np.float32).tobytes()


def test_guided_filter_converges_where_the_plain_one_does_not(blob):
    """RMSE against the oracle's 2048-spp seed-99 render, as a fraction of the noisy image's, default parameters.
    4 x 1 samples: the guided filter is at most 0.5 (measured 0.24; plain 0.23).  16 x 8 samples: the guided filter
    is below 1 (measured 0.83) while the plain filter is above 1 (measured 1.22) -- a filter that ignores `var`
    cannot meet both.  Over seeds 1234 / 7 / 42 the restatement measured 0.20-0.24 (guided) at 4 samples and
    0.64-0.83 (guided) against 1.15-1.22 (plain) at 128."""
    render, clean, feat = blob
    noisy, var = _progressive(render, 4, 1)
    assert np.isfinite(var).all() and (var > 0).any()
    e_noisy = denoise_ref.rmse(noisy, clean)
    e_guided = denoise_ref.rmse(denoise_guided_ref.denoise_guided_ref(noisy, feat, var), clean)
    print("4 x 1: rmse noisy %.4f guided %.4f ratio %.3f" % (e_noisy, e_guided, e_guided / e_noisy))
    assert e_guided <= 0.5 * e_noisy

    noisy, var = _progressive(render, 16, 8)
    out = denoise_guided_ref.denoise_guided_ref(noisy, feat, var)
    e_noisy = denoise_ref.rmse(noisy, clean)
    e_guided = denoise_ref.rmse(out, clean)
    e_plain = denoise_ref.rmse(denoise_ref.denoise_ref(noisy, feat), clean)
    print("16 x 8: rmse noisy %.4f guided %.4f (%.3f) plain %.4f (%.3f)"
          % (e_noisy, e_guided, e_guided / e_noisy, e_plain, e_plain / e_noisy))
    assert e_guided < e_noisy
    assert e_plain > e_noisy
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    assert skip.any() and out[skip].tobytes() == noisy[skip].tobytes()
