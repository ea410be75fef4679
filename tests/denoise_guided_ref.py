"""numpy restatement of the variance-guided denoiser (include/pt/pt.h, "the variance-guided denoiser") and of the
variance map of the image's mean (pt_noise_variance), for the tests: every operation is written out and rounded on
its own, in the header's order, so the GPU kernels are compared with it bit for bit.  It is denoise_ref's loop with
the header's additions; all images here are (H, W, ...) in scanline order.

    var = variance_ref(est, counts)             # est: noise_ref.NoiseRef or adaptive_ref.AdaptiveRef
    out = denoise_guided_ref(img, feat, var)
"""
import numpy as np

import cudapathtracer_amd as pt

import adaptive_ref
from denoise_ref import F, H5, _shift

G3 = [F(0.25), F(0.5), F(0.25)]     # g at -1..1
UNKNOWN = F(1e30)


def variance_ref(est, counts):
    """The float32 map of pt_noise_variance: m2 / ((b - 1) * n) in f64, +inf before two batches.  counts: every
    pixel's sample count n_q (an int for an estimator without frozen pixels)."""
    with np.errstate(all="ignore"):
        if isinstance(est, adaptive_ref.AdaptiveRef):
            n = np.asarray(counts).astype(np.float64)
            v = est.m2 / ((est.bq - np.uint32(1)).astype(np.float64) * n)
            return np.where(est.bq < 2, np.inf, v).astype(np.float32)
        if est.batches < 2:
            return np.full(est.mu.shape, np.inf, dtype=np.float32)
        return (est.m2 / (float(est.batches - 1) * float(int(counts)))).astype(np.float32)


def luma(c):
    return ((F(0.2126) * c[..., 0]) + (F(0.7152) * c[..., 1])) + (F(0.0722) * c[..., 2])


def denoise_guided_ref(img, feat, var, iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0, demodulate=True,
                       sigma_luma=2.0):
    img = np.ascontiguousarray(img, dtype=F)
    if iterations == 0:
        return img.copy()
    var = np.ascontiguousarray(var, dtype=F)
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    alb = feat["albedo"].astype(F)
    a = np.where(alb > F(1e-3), alb, F(1e-3)).astype(F) if demodulate else np.ones_like(alb)
    with np.errstate(all="ignore"):
        c = (img / a).astype(F)
        A = luma(a) if demodulate else np.ones(var.shape, dtype=F)
        t = var / (A * A)
        v = np.where((var >= 0) & (t < UNKNOWN), t, UNKNOWN).astype(F)
        n, P = feat["normal"].astype(F), feat["position"].astype(F)
        s = (F(sigma_depth) * feat["depth"].astype(F)).astype(F)
        one = F(1.0)
        sl2 = F(sigma_luma) * F(sigma_luma)
        for it in range(iterations):
            step = 1 << it
            lum = luma(c)
            va = np.zeros(s.shape, dtype=F)
            vw = np.zeros(s.shape, dtype=F)
            for j in range(-1, 2):
                for i in range(-1, 2):
                    vq, ok = _shift(v, i, j)
                    sq, _ = _shift(skip, i, j)
                    ok = ok & ~sq
                    g = G3[j + 1] * G3[i + 1]
                    va = np.where(ok, va + (g * vq), va)
                    vw = np.where(ok, vw + g, vw)
            den = (sl2 * (va / vw)) + F(1e-20)
            acc = [np.zeros(s.shape, dtype=F) for _ in range(3)]
            wsum = np.zeros(s.shape, dtype=F)
            vacc = np.zeros(s.shape, dtype=F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    nq, ok = _shift(n, i * step, j * step)
                    Pq, _ = _shift(P, i * step, j * step)
                    cq, _ = _shift(c, i * step, j * step)
                    lq, _ = _shift(lum, i * step, j * step)
                    vq, _ = _shift(v, i * step, j * step)
                    sq, _ = _shift(skip, i * step, j * step)
                    ok = ok & ~sq
                    dn = ((n[..., 0] * nq[..., 0]) + (n[..., 1] * nq[..., 1])) + (n[..., 2] * nq[..., 2])
                    dn = np.where(dn > 0, dn, F(0.0)).astype(F)
                    wn = dn
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    e = ((n[..., 0] * (Pq[..., 0] - P[..., 0])) + (n[..., 1] * (Pq[..., 1] - P[..., 1]))) + \
                        (n[..., 2] * (Pq[..., 2] - P[..., 2]))
                    r = e / s
                    wz = one / (one + (r * r))
                    wt = ((H5[j + 2] * H5[i + 2]) * wn) * wz
                    if sigma_color > 0:
                        d0, d1, d2 = (cq[..., k] - c[..., k] for k in range(3))
                        dc = ((d0 * d0) + (d1 * d1)) + (d2 * d2)
                        sc = F(sigma_color) / F(1 << it)
                        wt = wt * (one / (one + (dc / (sc * sc))))
                    dl = lq - lum
                    wt = wt * (one / (one + ((dl * dl) / den)))
                    assert wt.dtype == F
                    for k in range(3):
                        acc[k] = np.where(ok, acc[k] + (wt * cq[..., k]), acc[k])
                    wsum = np.where(ok, wsum + wt, wsum)
                    vacc = np.where(ok, vacc + ((wt * wt) * vq), vacc)
            good = (wsum > 0) & ~skip
            new = c.copy()
            for k in range(3):
                new[..., k] = np.where(good, acc[k] / wsum, c[..., k])
            v = np.where(good, vacc / (wsum * wsum), v).astype(F)
            c = new
        out = (c * a).astype(F)
    out[skip] = img[skip]
    return out
