"""Feature buffers and the preview denoiser without a GPU: the C-ABI's layouts, defaults and refusals, and the
numpy restatement of the filter (tests/denoise_ref.py) doing its job on the oracle's own render."""
import ctypes as C

import numpy as np

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, scenes

import denoise_ref


def test_feature_layout():
    assert C.sizeof(_lib.Feature) == 48 and pt.FEATURE.itemsize == 48
    for name, off in (("albedo", 0), ("depth", 12), ("normal", 16), ("prim", 28), ("position", 32), ("reserved", 44)):
        assert getattr(_lib.Feature, name).offset == off and pt.FEATURE.fields[name][1] == off
    assert C.sizeof(_lib.DenoiseParams) == 20
    assert pt.PT_FEATURE_EMISSIVE == 0x40000000 and pt.PT_DENOISE_NO_DEMODULATE == 1


def test_denoise_defaults():
    dp = _lib.DenoiseParams(-1, -1, -1.0, -1.0, 99)
    _lib.lib().pt_denoise_defaults(C.byref(dp))
    assert (dp.iterations, dp.normal_power_log2, dp.flags) == (5, 5, 0)
    assert dp.sigma_depth == np.float32(0.02) and dp.sigma_color == 0.0
    _lib.lib().pt_denoise_defaults(None)
    assert pt.denoise_defaults()["iterations"] == 5


def test_null_arguments_are_refused():
    L = _lib.lib()
    p = pt.Renderer.params(8, 8, 1)
    cam = pt.make_camera(width=8, height=8)
    dp = pt.Renderer.denoise_params()
    buf = np.zeros(8 * 8 * 12, dtype=np.float32)
    calls = [
        lambda: L.pt_render_features(None, C.byref(p), C.byref(cam), buf.ctypes.data),
        lambda: L.pt_render_features(None, None, None, None),
        lambda: L.pt_render_features_device(None, C.byref(p), C.byref(cam), buf.ctypes.data, None),
        lambda: L.pt_render_features_device(None, None, None, None, None),
        lambda: L.pt_denoise(None, C.byref(dp), 8, 8, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data),
        lambda: L.pt_denoise(None, None, 8, 8, 0, None, None, None),
        lambda: L.pt_denoise_device(None, C.byref(dp), 8, 8, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None),
        lambda: L.pt_denoise_device(None, None, 8, 8, 0, None, None, None, None),
    ]
    for call in calls:
        assert call() == _lib.PT_E_INVALID
        assert b"null" in L.pt_last_error()


def test_reference_filter_removes_noise():
    """The numpy reference on the oracle's 64x64 / 4-spp / seed-1234 cornell_blob render with oracle-traced
    features: its RMSE against the oracle's 2048-spp seed-99 render is at most 0.5x the noisy image's (measured
    0.23x), so the condition cannot hold for a filter that does nothing."""
    import oracle
    s = load_scene("cornell_blob")
    arrays = s.arrays()
    osc = oracle.OracleScene(arrays)
    w = h = 64
    kw = scenes.CORNELL_CAMERA
    ocam = oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], kw["radius"], w, h)
    noisy = oracle.render(osc, ocam, w, h, 4, 3, 0, 1234)[0].astype(np.float32)
    clean = oracle.render(osc, ocam, w, h, 2048, 3, 0, 99)[0].astype(np.float32)
    feat = denoise_ref.features_ref(arrays, pt.make_camera(width=w, height=h, **kw), w, h,
                                    lambda o, d: oracle.trace_batch(osc, o, d))
    assert (feat["prim"] < 0).any() or (feat["prim"] & pt.PT_FEATURE_EMISSIVE).any()
    out = denoise_ref.denoise_ref(noisy, feat)
    e_noisy, e_out = denoise_ref.rmse(noisy, clean), denoise_ref.rmse(out, clean)
    print("rmse noisy %.4f filtered %.4f ratio %.3f" % (e_noisy, e_out, e_out / e_noisy))
    assert e_out <= 0.5 * e_noisy
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    assert out[skip].tobytes() == noisy[skip].tobytes()
