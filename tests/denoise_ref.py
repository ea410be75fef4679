"""numpy float32 restatement of the preview denoiser (include/pt/pt.h, "The filter's arithmetic") and of the
primary-hit feature buffers, for the tests: every operation is written out and rounded on its own, in the
header's order, so the GPU kernels are compared with it bit for bit.  All images here are (H, W, ...) in
scanline order."""
import numpy as np

import cudapathtracer_amd as pt

F = np.float32
H5 = [F(1.0 / 16), F(1.0 / 4), F(3.0 / 8), F(1.0 / 4), F(1.0 / 16)]   # h at -2..2 (all exact in f32)
MAX_FLOAT = F(100000.0)


def features_ref(scene_arrays, cam, w, h, trace):
    """The (H, W) FEATURE array of pt_render_features, composed on the host: pt.camera_ray (no lens draws),
    `trace(origins, directions) -> (tri, t)` (oracle.trace_batch on the CPU, Renderer.trace on the GPU), then
    the scene arrays."""
    o = np.empty((h, w, 3), dtype=F)
    d = np.empty((h, w, 3), dtype=F)
    for y in range(h):
        for x in range(w):
            o[y, x], d[y, x] = pt.camera_ray(cam, pt.morton_pxl_to_i(x, y), False)
    tri, t = trace(o.reshape(-1, 3), d.reshape(-1, 3))
    tri = np.asarray(tri, dtype=np.int32).reshape(h, w)
    t = np.asarray(t, dtype=F).reshape(h, w)
    tris, mats, sph = scene_arrays["tris"], scene_arrays["mats"], scene_arrays["spheres"]
    nt = len(tris)
    f = np.zeros((h, w), dtype=pt.FEATURE)
    f["prim"] = -1
    f["depth"] = t
    for y in range(h):
        for x in range(w):
            k = int(tri[y, x])
            if k < 0:
                continue
            r = f[y, x]
            pos = (o[y, x] + (d[y, x] * t[y, x]).astype(F)).astype(F)
            if k < nt:
                alb, emi = mats[tris[k]["mat"]]["albedo"], mats[tris[k]["mat"]]["emission"]
                nrm = np.array([tris[k]["nx"], tris[k]["ny"], tris[k]["nz"]], dtype=F)
            else:
                s = sph[k - nt]
                alb, emi = s["diffuse"], s["emission"]
                nrm = ((pos - s["pos"].astype(F)).astype(F) / F(s["rad"])).astype(F)
            r["albedo"] = alb.astype(F)
            r["normal"] = nrm
            r["position"] = pos
            r["prim"] = k | (pt.PT_FEATURE_EMISSIVE if emi[0] != 0 else 0)
    return f


def _shift(a, dx, dy):
    """a[y + dy, x + dx] where inside the image (elsewhere: zeros), and the mask of those pixels."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), dtype=bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def denoise_ref(img, feat, iterations=5, normal_power_log2=5, sigma_depth=0.02, sigma_color=0.0, demodulate=True):
    img = np.ascontiguousarray(img, dtype=F)
    if iterations == 0:
        return img.copy()
    skip = (feat["prim"] < 0) | ((feat["prim"] & pt.PT_FEATURE_EMISSIVE) != 0)
    alb = feat["albedo"].astype(F)
    a = np.where(alb > F(1e-3), alb, F(1e-3)).astype(F) if demodulate else np.ones_like(alb)
    with np.errstate(all="ignore"):
        c = (img / a).astype(F)
        n, P = feat["normal"].astype(F), feat["position"].astype(F)
        s = (F(sigma_depth) * feat["depth"].astype(F)).astype(F)
        one = F(1.0)
        for it in range(iterations):
            step = 1 << it
            acc = [np.zeros(s.shape, dtype=F) for _ in range(3)]
            wsum = np.zeros(s.shape, dtype=F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    nq, ok = _shift(n, i * step, j * step)
                    Pq, _ = _shift(P, i * step, j * step)
                    cq, _ = _shift(c, i * step, j * step)
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
                    assert wt.dtype == F
                    for k in range(3):
                        acc[k] = np.where(ok, acc[k] + (wt * cq[..., k]), acc[k])
                    wsum = np.where(ok, wsum + wt, wsum)
            good = (wsum > 0) & ~skip
            new = c.copy()
            for k in range(3):
                new[..., k] = np.where(good, acc[k] / wsum, c[..., k])
            c = new
        out = (c * a).astype(F)
    out[skip] = img[skip]
    return out


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))
