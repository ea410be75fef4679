"""The noise estimator without a device: argument checks through the raw ABI, the numpy restatement
(tests/noise_ref.py) against the closed-form weighted variance, and the estimator's validity on oracle renders --
the estimated variance of the mean, summed over the image, against the variance actually seen across seeds."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib

import noise_ref

LUMA = (0.2126, 0.7152, 0.0722)


def test_null_arguments_and_defaults():
    L = _lib.lib()

    def msg():
        return (L.pt_last_error() or b"").decode()

    d = _lib.NoiseParams(-1.0, -1.0)
    L.pt_noise_defaults(C.byref(d))
    assert (d.tol, d.y_floor) == (np.float32(0.05), np.float32(0.01))
    assert pt.noise_defaults() == dict(tol=d.tol, y_floor=d.y_floor)
    L.pt_noise_defaults(None)
    err = C.c_int(0)
    assert not L.pt_noise_create(None, C.byref(err))
    assert err.value == _lib.PT_E_INVALID and "pt_noise_create" in msg()
    assert not L.pt_noise_create(None, None)
    s = _lib.NoiseSummary()
    assert L.pt_noise_update(None, C.byref(d), None, C.byref(s)) == _lib.PT_E_INVALID and "pt_noise_update" in msg()
    assert L.pt_noise_update(None, None, None, None) == _lib.PT_E_INVALID
    assert L.pt_noise_read(None, None, None) == _lib.PT_E_INVALID and "pt_noise_read" in msg()
    buf = (C.c_float * 4)()
    assert L.pt_noise_map(None, C.byref(d), buf) == _lib.PT_E_INVALID and "pt_noise_map" in msg()
    assert L.pt_noise_map(None, None, None) == _lib.PT_E_INVALID
    assert L.pt_noise_map_device(None, C.byref(d), buf, None) == _lib.PT_E_INVALID and "pt_noise_map_device" in msg()
    cp, res = _lib.ConvergeParams(), _lib.ConvergeResult()
    assert L.pt_accum_add_until(None, None, C.byref(cp), None, None, C.byref(res)) == _lib.PT_E_INVALID
    assert "pt_accum_add_until" in msg()
    L.pt_noise_destroy(None)


def _closed_form(samples, split, y_floor):
    """mu, m2, rel2 of the window in np.longdouble, from the per-sample values (N, P, 3) themselves."""
    ld = np.longdouble
    x = samples.astype(ld)
    lum = (ld(LUMA[0]) * x[..., 0] + ld(LUMA[1]) * x[..., 1]) + ld(LUMA[2]) * x[..., 2]
    edges = np.concatenate([[0], np.cumsum(split)])
    y = np.stack([lum[a:b].mean(axis=0) for a, b in zip(edges[:-1], edges[1:])])          # batch means
    s = np.array(split, dtype=ld)[:, None]
    W = s.sum()
    mu = (s * y).sum(axis=0) / W
    m2 = (s * (y - mu) ** 2).sum(axis=0)
    var = m2 / ((len(split) - 1) * W)
    den = np.maximum(ld(np.float32(y_floor)), mu)
    return mu, m2, var / (den * den)


@pytest.mark.parametrize("split", [[4, 1, 4], [2, 3, 4], [1] * 5, [3, 5]], ids=lambda s: "-".join(map(str, s)))
def test_restatement_equals_the_closed_form(split):
    rng = np.random.default_rng(20240611)
    P, N = 257, sum(split)
    samples = rng.random((N, P, 3)) * rng.random((1, P, 1)) * 4.0        # iid per pixel, pixel-dependent scale
    samples[:, 0, :] = 0.5                                               # a constant pixel
    samples[:, 1, :] = 0.0                                               # a zero pixel
    est = noise_ref.NoiseRef(0, shape=(P,))
    n = 0
    for k in split:
        n += k
        assert est.update(n, samples[:n].sum(axis=0) / float(n))         # the f64 running mean after n samples
    assert not est.update(n, samples[:n].sum(axis=0) / float(n))         # nothing new: nothing folded
    assert est.batches == len(split) and est.W == float(N)
    mu, m2, rel2 = _closed_form(samples, split, noise_ref.Y_FLOOR)

    def rel_err(a, b):
        b = b.astype(np.longdouble)
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))

    body = slice(2, None)
    assert rel_err(est.mu[body], mu[body]) <= 1e-12
    assert rel_err(est.m2[body], m2[body]) <= 1e-12
    assert rel_err(est.rel2()[body], rel2[body]) <= 1e-12
    # the constant pixel: every batch mean is the same double, so m2 is exactly 0; the zero pixel: all 0
    assert est.m2[0] == 0.0 and abs(est.mu[0] - 0.5) <= 1e-15 and est.rel2()[0] == 0.0
    assert est.mu[1] == 0.0 and est.m2[1] == 0.0 and est.rel2()[1] == 0.0
    s = est.summary(tol=1e-3)
    assert s["pixels"] == P and s["hist"][0] >= 2 and sum(s["hist"]) == P
    assert s["converged"] == int(np.count_nonzero(rel2 <= np.longdouble(np.float32(1e-3)) ** 2))


def test_bins_and_the_converged_rule():
    r = np.array([np.nan, 0.0, -1.0, np.inf, 1.0, 2.0 ** -47, 2.0 ** -48, 2.0 ** -100, 2.0 ** 14, 2.0 ** 15, 3.0e38,
                  1.0e-45], dtype=np.float32)
    assert list(noise_ref.bins(r)) == [63, 0, 0, 63, 48, 1, 1, 1, 62, 62, 62, 1]
    est = noise_ref.NoiseRef(0, shape=(3,))
    assert np.isinf(est.rel2()).all() and est.summary()["hist"][63] == 3 and est.summary()["converged"] == 0
    est.update(2, np.ones((3, 3)))
    assert np.isinf(est.rel2()).all() and est.summary(tol=1e30)["converged"] == 0     # one batch: inf, not converged


@pytest.mark.parametrize("integ", [0, 1])
def test_estimator_is_valid_on_oracle_renders(integ):
    """cornell_blob 32x32, 8 passes of 4 samples, bounces 3, seeds 1000..1023: the image sum of the estimated
    variance of the mean luminance (averaged over the seeds) over the image sum of the variance of the final mean
    luminance across the seeds.  Deterministic; measured 1.017 (integrator 0) and 0.995 (integrator 1), the worst
    8-seed subgroup 0.095 away from 1 -- the band is about twice that."""
    import oracle
    scene = load_scene("cornell_blob")
    osc = oracle.OracleScene(scene.arrays())
    w = h = 32
    ocam = oracle.camera((0.0, 1.0, 3.0), 1.0, 3.0, 0.0, w, h)
    est_var, final = [], []
    for seed in range(1000, 1024):
        est = noise_ref.NoiseRef(0, shape=(h, w))
        for n in range(4, 33, 4):
            img, _ = oracle.render(osc, ocam, w, h, n, 3, integ, seed)     # = the accumulator's mean64 after n samples
            est.update(n, img)
        assert est.batches == 8 and est.W == 32.0
        est_var.append(est.m2 / (float(est.batches - 1) * est.W))
        final.append(est.mu)
    ratio = float(np.mean(est_var, axis=0).sum() / np.var(final, axis=0, ddof=1).sum())
    print("integrator %d: estimated / empirical variance of the mean = %.4f" % (integ, ratio))
    assert 0.8 <= ratio <= 1.25, ratio
