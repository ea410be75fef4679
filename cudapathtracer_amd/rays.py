"""Ray sets for Renderer.render_rays (pt_render_rays) and point sets for Renderer.render_irradiance
(pt_render_irradiance): host only, numpy.

Every helper returns (origins, directions), two float32 arrays of shape (W*H, 3) in scanline order (the ray of pixel
(x, y) at y*W + x), the directions normalised in float32 -- so every ray is "regular" for a scene the origins lie
within 64 extents of, and the render takes the wavefront kernels.  For a Morton-ordered render permute the rows to
Morton order first.

The image orientation is the pinhole camera's: a set built at the camera's pose shows the scene the way
Renderer.render does (film x and y grow against the view's right and up, as camera.h's film does).

The point helpers (grid_points, triangle_points, chart_points, feature_points) return (points, normals) the same way, the normals
normalised in float32 and the points lifted `lift` along them: an irradiance render uses a point as given, and one
lying in its own surface is black.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import api, shard

F = np.float32


def _normalised(d):
    """Rows of d (float32) divided by their float32 length: x*x + y*y + z*z summed left to right, one square root."""
    d = np.ascontiguousarray(d, dtype=F)
    l2 = d[:, 0] * d[:, 0]
    l2 = l2 + d[:, 1] * d[:, 1]
    l2 = l2 + d[:, 2] * d[:, 2]
    ln = np.sqrt(l2)
    return np.ascontiguousarray(d / ln[:, None], dtype=F)


def _basis(pos, target, up):
    """(right, up, back), float64 unit vectors: the camera at pos looks along -back at target."""
    pos, target, up = (np.asarray(v, dtype=np.float64) for v in (pos, target, up))
    back = pos - target
    nb = np.linalg.norm(back)
    if not nb > 0:
        raise ValueError("rays: pos and target coincide")
    back = back / nb
    right = np.cross(up, back)
    nr = np.linalg.norm(right)
    if not nr > 0:
        raise ValueError("rays: up is parallel to the viewing direction")
    right = right / nr
    return right, np.cross(back, right), back


def _film(W, H):
    """The film coordinates of the pixel centres, (W*H,) each: ((x + 0.5) / W - 0.5, (y + 0.5) / H - 0.5), scanline."""
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError("rays: bad image size %dx%d" % (W, H))
    x = (np.arange(W, dtype=np.float64) + 0.5) / W - 0.5
    y = (np.arange(H, dtype=np.float64) + 0.5) / H - 0.5
    return np.tile(x, H), np.repeat(y, W)


def camera_rays(cam, view=None):
    """The camera's own pinhole rays: pt_camera_ray_view(cam, view, morton(x, y), lens = 0) per pixel of its
    pxl_width x pxl_height image, element for element.  render_rays over them equals render(cam, view=view) in every
    bit for a radius == 0 camera, except at pixel (0, 0) (there render() draws the reference's two quirk lens
    numbers per sample)."""
    W, H = int(cam.pxl_width), int(cam.pxl_height)
    if W <= 0 or H <= 0 or W > 65535 or H > 65535:
        raise ValueError("rays: bad image size %dx%d" % (W, H))
    ys, xs = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    idx = shard.morton_index(xs, ys).tolist()
    # (one library call per pixel, into one pair of vec3s: about a second per million pixels)
    call, cref, vref = L.lib().pt_camera_ray_view, C.byref(cam), api._view_ref(view)
    ov, dv = L.Vec3(), L.Vec3()
    oref, dref = C.byref(ov), C.byref(dv)
    rays = np.empty((W * H, 6), dtype=F)
    for k, i in enumerate(idx):
        call(cref, vref, i, 0, 0.0, 0.0, oref, dref)
        rays[k] = (ov.x, ov.y, ov.z, dv.x, dv.y, dv.z)
    return np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])


def ortho_rays(pos, target, up, film_w, film_h, W, H):
    """An orthographic projection: parallel rays along pos -> target from a film_w x film_h rectangle (scene units)
    centred on pos."""
    right, upv, back = _basis(pos, target, up)
    sx, sy = _film(W, H)
    o = np.asarray(pos, dtype=np.float64)[None, :] - sx[:, None] * float(film_w) * right - sy[:, None] * float(film_h) * upv
    d = np.broadcast_to(0.0 - back, o.shape)
    return np.ascontiguousarray(o, dtype=F), _normalised(d)


def panorama_rays(pos, W, H):
    """An equirectangular panorama from pos: longitude -pi..pi across the image (-z in the middle column, as the
    reference camera looks), latitude from straight up (row 0) to straight down."""
    sx, sy = _film(W, H)
    lon = 2.0 * np.pi * sx
    lat = np.pi * sy
    d = np.stack([-np.cos(lat) * np.sin(lon), -np.sin(lat), -np.cos(lat) * np.cos(lon)], axis=1)
    o = np.broadcast_to(np.asarray(pos, dtype=np.float64), d.shape)
    return np.ascontiguousarray(o, dtype=F), _normalised(d)


def fisheye_rays(pos, target, up, fov_deg, W, H):
    """An equidistant fisheye looking from pos at target: the angle from the axis grows linearly with the distance
    from the image centre and reaches fov_deg / 2 on the circle inscribed in the image; beyond pi it stays pi."""
    right, upv, back = _basis(pos, target, up)
    sx, sy = _film(W, H)
    m = float(min(int(W), int(H)))
    ux, uy = sx * (int(W) / m), sy * (int(H) / m)
    r = np.sqrt(ux * ux + uy * uy)
    ang = np.minimum(2.0 * r * np.radians(float(fov_deg)) / 2.0, np.pi)
    rs = np.where(r > 0, r, 1.0)
    lat = (-(ux / rs)[:, None] * right - (uy / rs)[:, None] * upv)   # unit vector in the film plane (0 at the centre)
    d = np.cos(ang)[:, None] * (0.0 - back) + np.sin(ang)[:, None] * lat
    o = np.broadcast_to(np.asarray(pos, dtype=np.float64), d.shape)
    return np.ascontiguousarray(o, dtype=F), _normalised(d)


def _lifted(p, n, lift):
    """(p + lift * n, n) as float32 (W*H, 3) arrays, n normalised in float32 first."""
    n = _normalised(n)
    p = np.asarray(p, dtype=np.float64) + float(lift) * n.astype(np.float64)
    return np.ascontiguousarray(p, dtype=F), n


def grid_points(corner, edge_u, edge_v, W, H, lift=1e-3):
    """Texel centres on the parallelogram corner + u * edge_u + v * edge_v, u = (x + 0.5) / W, v = (y + 0.5) / H, in
    scanline order; every normal is cross(edge_u, edge_v), normalised."""
    sx, sy = _film(W, H)
    c, eu, ev = (np.asarray(v, dtype=np.float64) for v in (corner, edge_u, edge_v))
    nrm = np.cross(eu, ev)
    if not np.linalg.norm(nrm) > 0:
        raise ValueError("rays: edge_u and edge_v are parallel")
    p = c[None, :] + (sx + 0.5)[:, None] * eu + (sy + 0.5)[:, None] * ev
    return _lifted(p, np.broadcast_to(nrm, p.shape), lift)


def triangle_points(arrays, tri, b1, b2, lift=1e-3):
    """Points v0 + b1 * (v1 - v0) + b2 * (v2 - v0) on triangles `tri` of Scene.arrays(), with the triangles' stored
    normals (normalised).  tri, b1, b2: one entry per point (scalars broadcast)."""
    tri = np.atleast_1d(np.asarray(tri, dtype=np.int64))
    b1 = np.broadcast_to(np.asarray(b1, dtype=np.float64), tri.shape)
    b2 = np.broadcast_to(np.asarray(b2, dtype=np.float64), tri.shape)
    t = arrays["tris"][tri]
    vx = np.stack([arrays["verts"][k].astype(np.float64) for k in ("x", "y", "z")], axis=1)
    v0, v1, v2 = vx[t["v0"]], vx[t["v1"]], vx[t["v2"]]
    p = v0 + b1[:, None] * (v1 - v0) + b2[:, None] * (v2 - v0)
    nrm = np.stack([t["nx"], t["ny"], t["nz"]], axis=1)
    return _lifted(p, nrm, lift)


def chart_points(arrays, tris, uvs, W, H, lift=1e-3):
    """Texel points of a UV chart: "bake this lightmap".  tris: T triangle indices of Scene.arrays(); uvs: (T, 3, 2),
    the chart coordinates of v0, v1, v2 in [0, 1]^2.  Texel (x, y) has centre c = ((x + 0.5) / W, (y + 0.5) / H); for
    triangle k in list order with chart corners a, b, cc, all in float64:
        e = b - a;  f = cc - a;  g = c - a;  det = e.x*f.y - e.y*f.x            (det == 0: the triangle is skipped)
        b1 = (g.x*f.y - g.y*f.x) / det;  b2 = (e.x*g.y - e.y*g.x) / det
    and the triangle covers the texel iff b1 >= 0, b2 >= 0 and b1 + b2 <= 1; the first covering triangle wins.
    Returns (points, normals, tri_of_texel, covered) in scanline order: a covered texel's point is
    triangle_points(arrays, tri, b1, b2, lift)'s; an uncovered one gets feature_points' dummy (the origin, normal +y),
    tri_of_texel = -1 and covered = False.  ~covered is the mask for Accumulator.freeze at 0 samples."""
    tris = np.atleast_1d(np.asarray(tris, dtype=np.int64))
    uvs = np.asarray(uvs, dtype=np.float64)
    if uvs.shape != (tris.shape[0], 3, 2):
        raise ValueError("rays: uvs must have shape (%d, 3, 2)" % tris.shape[0])
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError("rays: bad image size %dx%d" % (W, H))
    # (the centres as defined, one division each: _film's -0.5 and back is not exact below 0.25)
    cx = np.tile((np.arange(W, dtype=np.float64) + 0.5) / W, H)
    cy = np.repeat((np.arange(H, dtype=np.float64) + 0.5) / H, W)
    n = cx.shape[0]
    which = np.full(n, -1, dtype=np.int64)   # position in `tris` of the texel's triangle
    b1 = np.zeros(n, dtype=np.float64)
    b2 = np.zeros(n, dtype=np.float64)
    for k in range(tris.shape[0]):
        a, b, cc = uvs[k]
        ex, ey = b[0] - a[0], b[1] - a[1]
        fx, fy = cc[0] - a[0], cc[1] - a[1]
        det = ex * fy - ey * fx
        if det == 0:
            continue
        gx, gy = cx - a[0], cy - a[1]
        t1 = (gx * fy - gy * fx) / det
        t2 = (ex * gy - ey * gx) / det
        take = (which < 0) & (t1 >= 0) & (t2 >= 0) & (t1 + t2 <= 1)
        which[take] = k
        b1[take] = t1[take]
        b2[take] = t2[take]
    covered = which >= 0
    p = np.zeros((n, 3), dtype=F)
    nrm = np.tile(np.array([0.0, 1.0, 0.0], dtype=F), (n, 1))
    if covered.any():
        p[covered], nrm[covered] = triangle_points(arrays, tris[which[covered]], b1[covered], b2[covered], lift)
    tri_of_texel = np.where(covered, tris[np.maximum(which, 0)] if tris.shape[0] else -1, -1).astype(np.int64)
    return p, nrm, tri_of_texel, covered


def feature_points(features, lift=1e-3):
    """The primary-hit positions and normals of a feature buffer (Renderer.features / features_rays), flattened in
    the buffer's own order: "bake what this camera sees".  Returns (points, normals, miss): miss marks the pixels
    without a hit (prim < 0), whose entries are a valid dummy point, the origin with normal +y."""
    f = np.asarray(features).reshape(-1)
    miss = f["prim"] < 0
    nrm = np.where(miss[:, None], np.array([0.0, 1.0, 0.0], dtype=F), f["normal"]).astype(F)
    pos = np.where(miss[:, None], F(0.0), f["position"])
    p, n = _lifted(pos, nrm, lift)
    p[miss] = 0.0
    return p, n, miss


def chart_uv_table(num_tris, tris, uvs):
    """The chart coordinates Renderer.lightmap_shade looks a lightmap up with: a (num_tris, 6) float32 table whose row t
    holds (ua.x, ua.y, ub.x, ub.y, uc.x, uc.y), the chart coordinates of v0, v1, v2 of original triangle t, and NaN
    for every triangle of no chart.  tris, uvs: chart_points' arguments -- T triangle indices and their (T, 3, 2)
    coordinates; where a triangle is listed twice the first entry holds, as in chart_points."""
    tris = np.atleast_1d(np.asarray(tris, dtype=np.int64))
    uvs = np.asarray(uvs, dtype=np.float64)
    if uvs.shape != (tris.shape[0], 3, 2):
        raise ValueError("rays: uvs must have shape (%d, 3, 2)" % tris.shape[0])
    num_tris = int(num_tris)
    if tris.shape[0] and (tris.min() < 0 or tris.max() >= num_tris):
        raise ValueError("rays: a chart triangle is outside 0..%d" % (num_tris - 1))
    table = np.full((num_tris, 6), np.nan, dtype=F)
    for k in range(tris.shape[0] - 1, -1, -1):   # (backwards: the first entry of a triangle is written last)
        table[tris[k]] = uvs[k].reshape(6)
    return table


def point_features(points, normals, tri_of_texel):
    """The feature records of a bake's texels (chart_points' points, normals and tri_of_texel), for the a-trous filters
    (Renderer.denoise, denoise_guided) in texture space before the dilation: position and normal as given, albedo 1 and
    depth 1 (so demodulation changes nothing and the depth weight measures scene units), prim the texel's triangle and
    -1 where it is uncovered (the filters pass such a texel through and let it contribute to no neighbour).  Returns a
    FEATURE array shaped like tri_of_texel; reshape it to (H, W) for the filters."""
    tri = np.asarray(tri_of_texel, dtype=np.int64)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=F).reshape(-1, 3)
    if p.shape[0] != tri.size or n.shape[0] != tri.size:
        raise ValueError("rays: points, normals and tri_of_texel differ in length")
    if tri.size and tri.max() >= 2 ** 30:
        raise ValueError("rays: a triangle id does not fit a feature record")
    f = np.zeros(tri.size, dtype=api.FEATURE)
    f["albedo"] = F(1.0)
    f["depth"] = F(1.0)
    f["normal"] = n
    f["position"] = p
    f["prim"] = np.where(tri.reshape(-1) < 0, -1, tri.reshape(-1)).astype(np.int32)
    return f.reshape(tri.shape)
