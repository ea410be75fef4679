"""Reference for sub-pixel jitter (PT_FLAG_JITTER / PT_FLAG_JITTER_TENT, include/pt/pt.h): the offset and the jittered
camera ray restated in numpy float32, one rounded operation per line, for the NULL view and for a view, and the
oracle's per-pixel render loop (or_render, oracle/pt_oracle.c) restated around them as view_ref.render restates it
around the oriented ray: the two film-point draws come first in every sample.  The oracle library knows nothing of
jitter; only its RNG, its sin/cos and its two integrators are called.

Everything here works on numpy float32 SCALARS (an operation on two float32 scalars is one IEEE f32 operation), so a
64-sample render of a small image still takes about a second.

TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import functools

import numpy as np

import oracle
import view_ref

F = np.float32
JITTER, TENT = 0x40, 0x80          # PT_FLAG_JITTER, PT_FLAG_JITTER_TENT
BOX_FLAGS, TENT_FLAGS = JITTER, JITTER | TENT


def _tent(u):
    """The inverse CDF of the tent of half-width 1 about 0."""
    u = F(u)
    if u < F(0.5):
        t = F(2.0) * u
        t = np.sqrt(t)
        return F(t - F(1.0))
    t = F(2.0) * u
    t = F(2.0) - t
    t = np.sqrt(t)
    return F(F(1.0) - t)


def offset(flags, ua, ub):
    """(jx, jy), float32, of the draws (ua, ub); (0, 0) without the flag."""
    if not flags & JITTER:
        return F(0.0), F(0.0)
    if flags & TENT:
        return F(F(0.5) + _tent(ua)), F(F(0.5) + _tent(ub))
    return F(ua), F(ub)


def _sincos(theta):
    so, co = C.c_float(), C.c_float()
    oracle.lib().or_sincos(float(theta), C.byref(so), C.byref(co))
    return F(so.value), F(co.value)


def ray(cam, view, px, py, jx, jy, lens, u1=0.0, u2=0.0):
    """(origin, direction), two float32 triples: the ray of pixel (px, py) of `cam` = (pos, dist, focal, radius, W, H)
    through the film point (px + jx, py + jy); view = None (the reference camera) or (right, up, back, (film_w,
    film_h)).  lens: the sample drew the lens pair (u1, u2)."""
    pos, dist, focal, radius, W, H = cam
    pos = [F(c) for c in pos]
    dist, focal, radius = F(dist), F(focal), F(radius)
    sx = F(int(px))
    sx = sx + F(jx)
    sy = F(int(py))
    sy = sy + F(jy)
    fx = sx / F(int(W))
    fx = fx - F(0.5)
    fy = sy / F(int(H))
    fy = fy - F(0.5)
    fz = dist
    if view is not None:
        fx = fx * F(view[3][0])
        fy = fy * F(view[3][1])
    nf = -focal
    fx = fx * nf
    fx = fx / dist
    fy = fy * nf
    fy = fy / dist
    fz = fz * nf
    fz = fz / dist
    lo = [F(0.0), F(0.0), F(0.0)]
    if lens:
        r = np.sqrt(F(u1))
        r = radius * r
        theta = F((2 * 3.14159) * float(F(u2)))
        s, c = _sincos(theta)
        lo = [r * c, r * s, F(0.0)]
    c = [fx - lo[0], fy - lo[1], fz - lo[2]]
    if view is None:
        w = c
        o = [lo[k] + pos[k] for k in range(3)]
    else:
        R, U, B = ([F(v) for v in view[i]] for i in range(3))
        w, o = [], []
        for k in range(3):
            a = R[k] * c[0]
            b = U[k] * c[1]
            a = a + b
            b = B[k] * c[2]
            w.append(a + b)
            if lens:
                a = R[k] * lo[0]
                b = U[k] * lo[1]
                a = a + b
                o.append(a + pos[k])
            else:
                o.append(F(0.0) + pos[k])
    l2 = w[0] * w[0]
    t = w[1] * w[1]
    l2 = l2 + t
    t = w[2] * w[2]
    l2 = l2 + t
    ln = np.sqrt(l2)
    d = [w[k] / ln for k in range(3)]
    assert all(type(v) is F for v in o + d)
    return np.array(o, dtype=F), np.array(d, dtype=F)


def centre_rays(cam, view, W, H):
    """(origins, directions), float32 (W*H, 3), scanline order: the rays through the centres of the pixels' footprints
    (jx = jy = 0.5, no lens draws) -- what pt_render_features traces with PT_FLAG_JITTER."""
    o = np.empty((W * H, 3), dtype=F)
    d = np.empty((W * H, 3), dtype=F)
    for y in range(H):
        for x in range(W):
            o[y * W + x], d[y * W + x] = ray(cam, view, x, y, 0.5, 0.5, False)
    return o, d


def render(osc, cam, view, flags, spp, bounces=3, integrator=0, seed=1234, pixels=None, counts=None, return_counters=False,
           swap=False):
    """view_ref.render's loop with the two draws first: the f64 mean image (H, W, 3).  flags: the jitter bits (0: the
    unjittered render, with today's corner ray -- no draws, no additions).  pixels: iterable of y*W + x (default: all;
    the others stay 0).  counts: (H, W) per-pixel sample counts instead of spp.  return_counters: (image, dict(traces))
    instead.  swap: ua and ub exchanged -- a deliberately wrong restatement, for the test that shows it discriminates."""
    h = view_ref._integrators()
    pos, dist, focal, radius, W, H = cam
    out = np.zeros((H, W, 3), dtype=np.float64)
    if pixels is None:
        pixels = range(W * H)
    rng = oracle.OXorwow()
    cnt = oracle.OCounters()
    L = (C.c_double * 3)()
    jitter = bool(flags & JITTER)
    for pix in pixels:
        px, py = int(pix) % W, int(pix) // W
        idx = view_ref.morton(px, py)
        h.or_xorwow_init(seed, idx, C.byref(rng))
        lens = idx == 0 or float(F(radius)) != 0.0
        nspp = spp if counts is None else int(counts[py, px])
        if not lens and not jitter:
            o, d = ray(cam, view, px, py, 0.0, 0.0, False)
        mean = [0.0, 0.0, 0.0]
        for n in range(1, nspp + 1):
            jx = jy = F(0.0)
            if jitter:
                ua = h.or_uniform(C.byref(rng))
                ub = h.or_uniform(C.byref(rng))
                jx, jy = offset(flags, ub, ua) if swap else offset(flags, ua, ub)
            u1 = u2 = 0.0
            if lens:
                u1 = h.or_uniform(C.byref(rng))
                u2 = h.or_uniform(C.byref(rng))
            if lens or jitter:
                o, d = ray(cam, view, px, py, jx, jy, lens, u1, u2)
            ov = oracle.OVec3(float(o[0]), float(o[1]), float(o[2]))
            dv = oracle.OVec3(float(d[0]), float(d[1]), float(d[2]))
            if integrator == 1:
                h.or_radiance_head(C.byref(osc.c), ov, dv, C.byref(rng), C.byref(L), C.byref(cnt))
            else:
                h.or_radiance_unidir(C.byref(osc.c), ov, dv, int(bounces), C.byref(rng), C.byref(L), C.byref(cnt))
            fn1, fn = float(F(n - 1)), float(F(n))
            for ch in range(3):
                mean[ch] = (mean[ch] * fn1) / fn + L[ch] / fn
        out[py, px] = mean
    if return_counters:
        return out, dict(traces=int(cnt.traces))
    return out


@functools.lru_cache(maxsize=None)
def _cached(scene_key, cam, view, flags, spp, bounces, integrator, seed, swap):
    return render(_scenes[scene_key], cam, view, flags, spp, bounces, integrator, seed, return_counters=True, swap=swap)


_scenes = {}


def render_cached(scene_key, osc, cam, view, flags, spp, bounces=3, integrator=0, seed=1234, return_counters=False, swap=False):
    """render() of the whole image, computed once per distinct argument set and shared (treat it as read-only)."""
    _scenes[scene_key] = osc
    img, cnt = _cached(scene_key, cam, view, flags, spp, bounces, integrator, seed, swap)
    img.setflags(write=False)
    return (img, dict(cnt)) if return_counters else img


same_bits = view_ref.same_bits
