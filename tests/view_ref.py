"""Reference for the oriented camera (pt_view, include/pt/pt.h): the ray arithmetic restated in numpy float32, one
rounded operation per line, and the oracle's per-pixel render loop (or_render, oracle/pt_oracle.c) restated around
it -- the oracle library itself knows nothing of views; only its RNG, its sin/cos and its two integrators are called.

TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import functools

import numpy as np

import oracle

F = np.float32

# the views the tests share: (right, up, back, film)
IDENTITY = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1))
# an exact 90-degree yaw about +y: the camera looks along -x (back = +x); axis swap with a sign flip, many exact zeros
YAW90 = ((0, 0, -1), (0, 1, 0), (1, 0, 0), (1, 1))
# the identity with +x mirrored: a left-handed basis
MIRROR = ((-1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1))


def look_at64(pos, target, up):
    """pt_view_look_at restated in float64 from the float32 inputs: (right, up', back) as float32 triples."""
    p = np.asarray(pos, dtype=F).astype(np.float64)
    t = np.asarray(target, dtype=F).astype(np.float64)
    u = np.asarray(up, dtype=F).astype(np.float64)
    b = p - t
    bl = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
    back = b / bl
    r = np.array([u[1] * back[2] - u[2] * back[1], u[2] * back[0] - u[0] * back[2], u[0] * back[1] - u[1] * back[0]])
    rl = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    right = r / rl
    up2 = np.array([back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2],
                    back[0] * right[1] - back[1] * right[0]])
    return right.astype(F), up2.astype(F), back.astype(F)


def generic(pos=(0.0, 1.0, 3.0)):
    """A generic look-at view from `pos`: no component of the basis is 0 or 1."""
    r, u, b = look_at64(pos, (0.3, 0.7, -0.2), (0.1, 1.0, 0.05))
    return (tuple(float(v) for v in r), tuple(float(v) for v in u), tuple(float(v) for v in b), (1, 1))


def with_film(view, film):
    return (view[0], view[1], view[2], tuple(film))


def fov_film(dist_from_film, vfov_deg, width, height):
    """pt_view_set_fov restated in float64 from the float32 inputs: the film (w, h) of a vertical field of view with
    square pixels, each rounded to float32 once."""
    half = (float(F(vfov_deg)) * 3.14159265358979323846) / 360.0
    fh = (2.0 * float(F(dist_from_film))) * np.tan(half)
    fw = (fh * float(width)) / float(height)
    return (float(F(fw)), float(F(fh)))


def _scaled(v, s):
    return tuple(float(F(F(c) * F(s))) for c in v)


def _negated(v):
    return tuple(-float(c) for c in v)


def _extra_shots():
    pos = (0.0, 1.0, 3.0)                      # the reference camera's position: in front of the box's open side
    inside = (0.6, 1.0, 0.3)                   # inside the box
    g = generic(pos)
    # the basis' squared lengths 9e-4 off 1, one above and one below: pt_view_validate's terms right.right - 1 and
    # up.up - 1 at nine tenths of its limit of 1e-3
    slack = (_scaled(g[0], np.sqrt(1.0 + 9e-4)), _scaled(g[1], np.sqrt(1.0 - 9e-4)), g[2], (1, 1))
    return {
        # the reference pose with +x mirrored: a left-handed basis
        "mirror": (pos, 1.0, 3.0, MIRROR),
        # a 90-degree roll about the viewing axis: right = +y, up = -x, back = +z
        "roll90": (pos, 1.0, 3.0, ((0, 1, 0), (-1, 0, 0), (0, 0, 1), (1, 1))),
        # under the box's ceiling, looking straight down -y (back = +y) with the roll of the x axis: many exact zeros
        "down": ((0.0, 1.9, 0.0), 1.0, 3.0, ((1, 0, 0), (0, 0, -1), (0, 1, 0), (1, 1))),
        # generic turned round (back negated, and right for handedness): it looks away from the scene, every ray misses
        "away": (pos, 1.0, 3.0, (_negated(g[0]), g[1], _negated(g[2]), (1, 1))),
        "slack": (pos, 1.0, 3.0, slack),
        # a very wide film: grazing directions with tiny components (from inside the box, where such rays still meet a
        # wall: from the reference position all but the centre pixels would miss); a very narrow one: all pixels nearly
        # one direction
        "wide": (inside, 1.0, 3.0, with_film(generic(inside), (64, 48))),
        "narrow": (pos, 1.0, 3.0, with_film(g, (2.0 ** -6, 2.0 ** -6))),
        # pt.look_at(..., vfov=35, cam=cam) of a 24 x 16 (or any 3:2) camera
        "fov": (pos, 1.0, 3.0, with_film(g, fov_film(1.0, 35.0, 24, 16))),
    }


# named shots (pos, dist_from_film, focal_length, view), usable with any scene that fits in about [-2, 2]^3
SHOTS_EXTRA = _extra_shots()


def far_pose(m):
    """(pos, dist_from_film, focal_length, view) of an oblique camera whose largest coordinate is -x = -m, looking at
    (0, 1, 0), with the field of view narrowed so that a box of extent 2 fills the frame (focal_length = the distance,
    dist_from_film a third of it, as the far cameras of test_gpu_ray_ranges.py)."""
    m = float(F(m))
    pos = tuple(float(F(c)) for c in (-m, 0.5 * m + 1.0, 0.25 * m))
    target = (0.0, 1.0, 0.0)
    focal = float(np.sqrt(sum((p - t) ** 2 for p, t in zip(pos, target))))
    r, u, b = look_at64(pos, target, (0.1, 1.0, 0.05))
    view = (tuple(float(v) for v in r), tuple(float(v) for v in u), tuple(float(v) for v in b), (1, 1))
    return pos, float(F(focal / 3.0)), float(F(focal)), view


def _sincos(theta):
    s, c = np.empty(theta.shape, dtype=F), np.empty(theta.shape, dtype=F)
    so, co = C.c_float(), C.c_float()
    f = oracle.lib().or_sincos
    for i, t in enumerate(theta):
        f(float(t), C.byref(so), C.byref(co))
        s[i], c[i] = so.value, co.value
    return s, c


def rays(cam, view, px, py, lens, u1=None, u2=None):
    """(origins, directions), float32 (n, 3): the rays of pixels (px[i], py[i]) of `cam` = (pos, dist, focal, radius,
    W, H) through `view` = (right, up, back, (film_w, film_h)).  lens: one flag for all; u1, u2 the lens draws."""
    pos, dist, focal, radius, W, H = cam
    pos = np.asarray(pos, dtype=F)
    dist, focal, radius = F(dist), F(focal), F(radius)
    R, U, B = (np.asarray(v, dtype=F) for v in view[:3])
    film_w, film_h = F(view[3][0]), F(view[3][1])
    px = np.asarray(px, dtype=np.uint32).reshape(-1)
    py = np.asarray(py, dtype=np.uint32).reshape(-1)
    n = len(px)
    fx = px.astype(F) / F(W)
    fx = fx - F(0.5)
    fx = fx * film_w
    fy = py.astype(F) / F(H)
    fy = fy - F(0.5)
    fy = fy * film_h
    fz = np.full(n, dist, dtype=F)
    nf = -focal
    fx = fx * nf
    fx = fx / dist
    fy = fy * nf
    fy = fy / dist
    fz = fz * nf
    fz = fz / dist
    lox = np.zeros(n, dtype=F)
    loy = np.zeros(n, dtype=F)
    loz = np.zeros(n, dtype=F)
    if lens:
        u1 = np.asarray(u1, dtype=F).reshape(-1)
        u2 = np.asarray(u2, dtype=F).reshape(-1)
        r = radius * np.sqrt(u1)
        theta = ((2 * 3.14159) * u2.astype(np.float64)).astype(F)
        s, c = _sincos(theta)
        lox = r * c
        loy = r * s
    cx = fx - lox
    cy = fy - loy
    cz = fz - loz
    w = np.empty((n, 3), dtype=F)
    for k in range(3):
        a = R[k] * cx
        b = U[k] * cy
        a = a + b
        b = B[k] * cz
        w[:, k] = a + b
    l2 = w[:, 0] * w[:, 0]
    t = w[:, 1] * w[:, 1]
    l2 = l2 + t
    t = w[:, 2] * w[:, 2]
    l2 = l2 + t
    ln = np.sqrt(l2)
    d = np.empty((n, 3), dtype=F)
    o = np.empty((n, 3), dtype=F)
    for k in range(3):
        d[:, k] = w[:, k] / ln
        if lens:
            a = R[k] * lox
            b = U[k] * loy
            a = a + b
            o[:, k] = a + pos[k]
        else:
            o[:, k] = F(0.0) + pos[k]
    assert o.dtype == F and d.dtype == F
    return o, d


def morton(x, y):
    r = 0
    for b in range(16):
        r |= ((x >> b) & 1) << (2 * b)
        r |= ((y >> b) & 1) << (2 * b + 1)
    return r


def morton_xy(idx):
    x = y = 0
    for b in range(16):
        x |= ((idx >> (2 * b)) & 1) << b
        y |= ((idx >> (2 * b + 1)) & 1) << b
    return x, y


def _integrators():
    """The oracle library; oracle.py sets the ctypes signatures of its two integrators."""
    return oracle.lib()


def render(osc, cam, view, spp, bounces=3, integrator=0, seed=1234, pixels=None, counts=None, tri_counts=None,
           return_counters=False):
    """or_render's per-pixel loop with the oriented ray: the f64 mean image (H, W, 3).  pixels: iterable of y*W + x
    (default: all; the others stay 0).  counts: (H, W) per-pixel sample counts instead of spp.  tri_counts: optional
    uint32[num_tris] array the integrators add their per-triangle test counts to (OCounters.tri_counts, as
    oracle.render).  return_counters: return (image, dict(traces, node_tests, tri_tests)) instead."""
    h = _integrators()
    pos, dist, focal, radius, W, H = cam
    out = np.zeros((H, W, 3), dtype=np.float64)
    if pixels is None:
        pixels = range(W * H)
    rng = oracle.OXorwow()
    cnt = oracle.OCounters()
    if tri_counts is not None:
        assert tri_counts.dtype == np.uint32 and tri_counts.flags.c_contiguous and len(tri_counts) == osc.c.num_tris
        cnt.tri_counts = tri_counts.ctypes.data
    L = (C.c_double * 3)()
    for pix in pixels:
        px, py = int(pix) % W, int(pix) // W
        idx = morton(px, py)
        h.or_xorwow_init(seed, idx, C.byref(rng))
        lens = idx == 0 or float(F(radius)) != 0.0
        nspp = spp if counts is None else int(counts[py, px])
        if not lens:
            o, d = rays(cam, view, [px], [py], False)
        mean = [0.0, 0.0, 0.0]
        for n in range(1, nspp + 1):
            if lens:
                u1 = h.or_uniform(C.byref(rng))
                u2 = h.or_uniform(C.byref(rng))
                o, d = rays(cam, view, [px], [py], True, [u1], [u2])
            ov = oracle.OVec3(float(o[0, 0]), float(o[0, 1]), float(o[0, 2]))
            dv = oracle.OVec3(float(d[0, 0]), float(d[0, 1]), float(d[0, 2]))
            if integrator == 1:
                h.or_radiance_head(C.byref(osc.c), ov, dv, C.byref(rng), C.byref(L), C.byref(cnt))
            else:
                h.or_radiance_unidir(C.byref(osc.c), ov, dv, int(bounces), C.byref(rng), C.byref(L), C.byref(cnt))
            fn1, fn = float(F(n - 1)), float(F(n))
            for ch in range(3):
                mean[ch] = (mean[ch] * fn1) / fn + L[ch] / fn
        out[py, px] = mean
    if return_counters:
        return out, dict(traces=int(cnt.traces), node_tests=int(cnt.node_tests), tri_tests=int(cnt.tri_tests))
    return out


@functools.lru_cache(maxsize=None)
def _cached(scene_key, cam, view, spp, bounces, integrator, seed):
    return render(_scenes[scene_key], cam, view, spp, bounces, integrator, seed, return_counters=True)


_scenes = {}


def render_cached(scene_key, osc, cam, view, spp, bounces=3, integrator=0, seed=1234, return_counters=False):
    """render() of the whole image, computed once per distinct argument set and shared (treat it as read-only).
    return_counters: (image, a copy of the oracle's counters) instead."""
    _scenes[scene_key] = osc
    img, cnt = _cached(scene_key, cam, view, spp, bounces, integrator, seed)
    img.setflags(write=False)
    return (img, dict(cnt)) if return_counters else img


def same_bits(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int(np.count_nonzero(a.view(u) != b.view(u)))
