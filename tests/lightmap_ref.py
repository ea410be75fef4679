"""The two lightmap rules of include/pt/pt.h (pt_lightmap_dilate, pt_lightmap_shade) restated in numpy: the gutter fill
as the plain (2r+1)^2 scan in the rule's own order, the lookup operation by operation in np.float32.  The GPU kernels
are compared with these in every bit (test_gpu_lightmap.py); test_lightmap_host.py checks them against hand-worked
cases.  Also the case data both test files share: masks, charts, odd-valued images."""
import numpy as np

F = np.float32
PT_FEATURE_EMISSIVE = 0x40000000
NO_ALBEDO = 0x1

# the classes of a shaded record: the six ways to `fill`, and a looked-up value
MISS, EMISSIVE, SPHERE, NO_CHART, DET, ST, SHADED = range(7)
FILL_CLASSES = (MISS, EMISSIVE, SPHERE, NO_CHART, DET, ST)


def offsets(radius):
    """The window's offsets (i, j) in the order the rule prefers them: smallest i*i + j*j, then smaller j, then
    smaller i."""
    o = [(i * i + j * j, j, i) for j in range(-radius, radius + 1) for i in range(-radius, radius + 1)]
    return [(i, j) for _, j, i in sorted(o)]


def dilate(img, covered, radius):
    """(out, src): every uncovered texel scans its window in the rule's order and takes the first covered texel inside
    the image; bits are moved as uint32, never as floats."""
    img = np.ascontiguousarray(img, dtype=F)
    H, W = img.shape[:2]
    cov = np.asarray(covered).reshape(H, W) != 0
    bits = img.view(np.uint32).reshape(H, W, 3)
    out = bits.copy()
    idx = np.arange(W * H, dtype=np.int64).reshape(H, W)
    src = np.where(cov, idx, -1)
    todo = ~cov
    ys, xs = np.mgrid[0:H, 0:W]
    for i, j in offsets(radius):
        if not todo.any():
            break
        xq, yq = xs + i, ys + j
        inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
        hit = todo & inside
        hit[hit] = cov[yq[hit], xq[hit]]
        out[hit] = bits[yq[hit], xq[hit]]
        src[hit] = idx[yq[hit], xq[hit]]
        todo &= ~hit
    return out.view(F), src.astype(np.int32)


def dilate_scalar(img, covered, radius):
    """dilate() texel by texel, tap by tap: the rule as it reads (for small images)."""
    img = np.ascontiguousarray(img, dtype=F)
    H, W = img.shape[:2]
    cov = np.asarray(covered).reshape(H, W) != 0
    bits = img.view(np.uint32).reshape(H, W, 3)
    out = bits.copy()
    src = np.full((H, W), -1, dtype=np.int32)
    for y in range(H):
        for x in range(W):
            if cov[y, x]:
                src[y, x] = y * W + x
                continue
            best = None
            for j in range(-radius, radius + 1):
                for i in range(-radius, radius + 1):
                    if 0 <= x + i < W and 0 <= y + j < H and cov[y + j, x + i]:
                        key = (i * i + j * j, j, i)
                        if best is None or key < best:
                            best = key
            if best is not None:
                _, j, i = best
                out[y, x] = bits[y + j, x + i]
                src[y, x] = (y + j) * W + (x + i)
    return out.view(F), src


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(F)


def shade(features, tri_uv, lightmap, arrays, fill=(0.0, 0.0, 0.0), flags=0):
    """(out, cls): pt_lightmap_shade over the records of `features` (any shape), operation by operation in float32, and
    the class of every record.  arrays: Scene.arrays() of the renderer's scene."""
    f = np.asarray(features)
    shape = f.shape
    f = f.reshape(-1)
    n = f.shape[0]
    uv = np.ascontiguousarray(tri_uv, dtype=F).reshape(-1, 6)
    lm = np.ascontiguousarray(lightmap, dtype=F)
    mh, mw = lm.shape[:2]
    tris, verts = arrays["tris"], arrays["verts"]
    nt = tris.shape[0]
    out = np.empty((n, 3), dtype=F)
    out[:] = np.asarray(fill, dtype=F)
    cls = np.full(n, SHADED, dtype=np.int64)
    prim = f["prim"].astype(np.int64)
    cls[prim >= nt] = SPHERE
    cls[(prim >= 0) & ((prim & PT_FEATURE_EMISSIVE) != 0)] = EMISSIVE
    cls[prim < 0] = MISS
    go = cls == SHADED
    t = np.where(go, prim, 0)
    if nt == 0:
        return out.reshape(shape + (3,)), cls.reshape(shape)
    row = uv[t]
    nochart = go & np.isnan(row[:, 0])
    cls[nochart] = NO_CHART
    go &= ~nochart
    vx = np.stack([verts["x"], verts["y"], verts["z"]], axis=1).astype(F)
    v0, v1, v2 = vx[tris["v0"][t]], vx[tris["v1"][t]], vx[tris["v2"][t]]
    with np.errstate(all="ignore"):
        e1 = [(v1[:, k] - v0[:, k]).astype(F) for k in range(3)]
        e2 = [(v2[:, k] - v0[:, k]).astype(F) for k in range(3)]
        g = [(f["position"][:, k].astype(F) - v0[:, k]).astype(F) for k in range(3)]
        d11, d12, d22, g1, g2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(g, e1), _dot(g, e2)
        det = d11 * d22 - d12 * d12
        bad = go & ((det == 0) | ~np.isfinite(det))
        cls[bad] = DET
        go &= ~bad
        b1 = _clamp((d22 * g1 - d12 * g2) / det, F(0), F(1))
        b2 = _clamp((d11 * g2 - d12 * g1) / det, F(0), F(1))
        u = (row[:, 0] + b1 * (row[:, 2] - row[:, 0])) + b2 * (row[:, 4] - row[:, 0])
        v = (row[:, 1] + b1 * (row[:, 3] - row[:, 1])) + b2 * (row[:, 5] - row[:, 1])
        s = u * F(mw) - F(0.5)
        tt = v * F(mh) - F(0.5)
        assert all(a.dtype == F for a in (det, b1, b2, u, v, s, tt))
        bad = go & ~(np.isfinite(s) & np.isfinite(tt))
        cls[bad] = ST
        go &= ~bad
        s = _clamp(np.where(go, s, F(0)), F(-1), F(mw))
        tt = _clamp(np.where(go, tt, F(0)), F(-1), F(mh))
        x0, y0 = np.floor(s), np.floor(tt)
        fx, fy = (s - x0).astype(F), (tt - y0).astype(F)
        xa, xb = np.clip(x0.astype(np.int64), 0, mw - 1), np.clip(x0.astype(np.int64) + 1, 0, mw - 1)
        ya, yb = np.clip(y0.astype(np.int64), 0, mh - 1), np.clip(y0.astype(np.int64) + 1, 0, mh - 1)
        for k in range(3):
            l00, l10, l01, l11 = lm[ya, xa, k], lm[ya, xb, k], lm[yb, xa, k], lm[yb, xb, k]
            top = l00 + fx * (l10 - l00)
            bot = l01 + fx * (l11 - l01)
            val = top + fy * (bot - top)
            res = val if (flags & NO_ALBEDO) else f["albedo"][:, k].astype(F) * val
            assert res.dtype == F
            out[go, k] = res[go]
    return out.reshape(shape + (3,)), cls.reshape(shape)


# ---- case data
def odd_image(W, H, seed):
    """A W x H x 3 float32 image of random bit patterns, with NaNs of several payloads, -0, infinities and denormals
    among them."""
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 2 ** 32, size=(H, W, 3), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001,
                        0x807fffff], dtype=np.uint32)
    pick = rng.randint(0, 3, size=(H, W, 3)) == 0
    bits[pick] = special[rng.randint(0, special.shape[0], size=int(pick.sum()))]
    return bits.view(F)


def masks(W, H, radius, seed):
    """name -> (H, W) uint8 mask: the cases of the dilation test."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    m = {"all": np.ones((H, W), np.uint8), "none": np.zeros((H, W), np.uint8)}
    c = np.zeros((H, W), np.uint8)
    c[0, 0] = c[0, W - 1] = c[H - 1, 0] = c[H - 1, W - 1] = 1
    m["corners"] = c
    m["checker"] = ((xs + ys) & 1).astype(np.uint8)
    m["checker3"] = (((xs // 3) + (ys // 3)) & 1).astype(np.uint8) * 255
    m["half"] = (rng.rand(H, W) < 0.5).astype(np.uint8)
    m["sparse"] = (rng.rand(H, W) < 0.02).astype(np.uint8) * 7
    col0 = np.zeros((H, W), np.uint8)
    col0[:, 0] = 1
    m["column0"] = col0
    colw = np.zeros((H, W), np.uint8)
    colw[:, W - 1] = 1
    m["columnW"] = colw
    one = np.zeros((H, W), np.uint8)
    one[H - 1, W - 1] = 1           # the texel `radius` up and left of it finds it, the one radius + 1 away does not
    m["one"] = one
    return m


def cornell_chart(arrays, lo=0.1, hi=0.9):
    """The Cornell floor (stored normal +y, at the scene's lowest y) charted by its own x, z over [-1, 1]^2 onto
    [lo, hi]^2, and the wall at the scene's lowest x charted by its z, y onto the whole [0, 1]^2 -- its chart
    coordinates reach 0 and 1 exactly.  Returns (tris, uvs) as rays.chart_points takes them, and the floor's ids."""
    t, v = arrays["tris"], arrays["verts"]
    ymin, ymax, xmin = float(v["y"].min()), float(v["y"].max()), float(v["x"].min())
    zmin, zmax = float(v["z"].min()), float(v["z"].max())
    corners = ("v0", "v1", "v2")
    floor = [k for k in range(len(t)) if t[k]["ny"] > 0.9 and all(abs(float(v["y"][t[k][c]]) - ymin) < 1e-6 for c in corners)]
    wall = [k for k in range(len(t)) if abs(t[k]["nx"]) > 0.9 and all(abs(float(v["x"][t[k][c]]) - xmin) < 1e-6 for c in corners)]
    assert floor and wall
    uv = np.zeros((len(floor) + len(wall), 3, 2), dtype=np.float64)
    half = 0.5 * (hi - lo)
    for i, k in enumerate(floor):
        for j, c in enumerate(corners):
            uv[i, j] = (0.5 + half * float(v["x"][t[k][c]]), 0.5 + half * float(v["z"][t[k][c]]))
    for i, k in enumerate(wall):
        for j, c in enumerate(corners):
            uv[len(floor) + i, j] = ((float(v["z"][t[k][c]]) - zmin) / (zmax - zmin), (float(v["y"][t[k][c]]) - ymin) / (ymax - ymin))
    return np.array(floor + wall, dtype=np.int64), uv, np.array(floor, dtype=np.int64)
