"""Reference for temporal reprojection (pt_project_view, pt_temporal_*; include/pt/pt.h): the header's arithmetic
restated in numpy float32, one rounded operation per line, vectorised over the image.  TemporalRef keeps the history
between pushes as the library's object does, and records in `stats` which branches a push took, so a test can assert
that its inputs reached them.

Cameras are (pos, dist_from_film, focal_length, radius, W, H) and views (right, up, back, (film_w, film_h)) or None,
as in view_ref.py; images and features are in scanline order.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

F = np.float32
IDENTITY = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1))
PT_FLAG_JITTER = 0x40
SNAP = F(0.015625)


def view_tuple(v):
    """The tuple form of a ctypes pt_view (or None)."""
    if v is None:
        return None
    return (tuple(float(c) for c in v.right), tuple(float(c) for c in v.up), tuple(float(c) for c in v.back),
            (float(v.film_w), float(v.film_h)))


def cam_tuple(c):
    """The tuple form of a ctypes pt_camera."""
    return ((float(c.pos.x), float(c.pos.y), float(c.pos.z)), float(c.dist_from_film), float(c.focal_length), float(c.radius),
            int(c.pxl_width), int(c.pxl_height))


def project(cam, view, P):
    """pt_project_view for points P (..., 3) float32: (front bool, sx, sy float32), each shaped like P without its last
    axis.  Where front is False, sx and sy are whatever the arithmetic gives (inf and NaN included)."""
    pos, dist, _, _, W, H = cam
    R, U, B, film = IDENTITY if view is None else view
    pos = [F(c) for c in pos]
    R, U, B = [F(c) for c in R], [F(c) for c in U], [F(c) for c in B]
    dist, fw, fh = F(dist), F(film[0]), F(film[1])
    P = np.asarray(P, dtype=F)
    qx = P[..., 0] - pos[0]
    qy = P[..., 1] - pos[1]
    qz = P[..., 2] - pos[2]

    def dot(v):
        a = v[0] * qx
        b = v[1] * qy
        a = a + b
        b = v[2] * qz
        return a + b

    cx, cy, cz = dot(R), dot(U), dot(B)
    front = cz < F(0)
    with np.errstate(all="ignore"):
        gx = cx * dist
        gx = gx / cz
        gy = cy * dist
        gy = gy / cz
        sx = gx / fw
        sx = sx + F(0.5)
        sx = sx * F(W)
        sy = gy / fh
        sy = sy + F(0.5)
        sy = sy * F(H)
    assert sx.dtype == F and sy.dtype == F
    return front, sx, sy


def _snap(f):
    with np.errstate(all="ignore"):
        r = np.floor(f + F(0.5))
        d = np.abs(f - r)
    near = d <= SNAP
    return np.where(near, r, f).astype(F), near


def lum(c):
    a = F(0.2126) * c[..., 0]
    b = F(0.7152) * c[..., 1]
    a = a + b
    b = F(0.0722) * c[..., 2]
    return a + b


# ---- the look-at orbit the host and GPU tests share: the camera circles (0, 1, 0) at the reference camera's distance
ORBIT_TARGET, ORBIT_UP, ORBIT_STEP = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.02   # radians per frame: under a pixel at 64x64
ORBIT_FRAMES, ORBIT_SIZE, ORBIT_SEED, ORBIT_REF_SPP = 8, 64, 1234, 2048
ORBIT_GOLDEN = "temporal_orbit_2048.npy"   # under tests/golden: the oracle's ORBIT_REF_SPP render of the last pose


def orbit_pose(i, step=ORBIT_STEP):
    """(pos, view) of frame i: float32-representable position, view as pt_view_look_at gives it (view_ref.look_at64)."""
    import view_ref
    th = step * i
    pos = (float(F(3.0 * np.sin(th))), 1.0, float(F(3.0 * np.cos(th))))
    r, u, b = view_ref.look_at64(pos, ORBIT_TARGET, ORBIT_UP)
    return pos, (tuple(float(v) for v in r), tuple(float(v) for v in u), tuple(float(v) for v in b), (1, 1))


def features_ref(arrays, cam, view, trace):
    """The (H, W) feature records of pt_render_features_view for a scene of triangles, composed on the host: the
    oriented corner rays (view_ref.rays), `trace(origins, directions) -> (prim, t)`, then the scene arrays."""
    import cudapathtracer_amd as pt
    import view_ref
    assert len(arrays["spheres"]) == 0
    w, h = cam[4], cam[5]
    ys, xs = np.mgrid[0:h, 0:w]
    o, d = view_ref.rays(cam, view, xs.reshape(-1), ys.reshape(-1), False)
    prim, t = trace(o, d)
    prim = np.asarray(prim, dtype=np.int32)
    t = np.asarray(t, dtype=F)
    hit = prim >= 0
    tris, mats = arrays["tris"], arrays["mats"]
    tk = tris[np.where(hit, prim, 0)]
    f = np.zeros(w * h, dtype=pt.FEATURE)
    f["depth"] = t
    for k in range(3):
        step = d[:, k] * t
        f["position"][:, k] = np.where(hit, o[:, k] + step, F(0))
        f["normal"][:, k] = np.where(hit, tk[("nx", "ny", "nz")[k]], F(0))
        f["albedo"][:, k] = np.where(hit, mats["albedo"][tk["mat"], k].astype(F), F(0))
    emissive = mats["emission"][tk["mat"], 0] != 0
    f["prim"] = np.where(hit, prim | np.where(emissive, pt.PT_FEATURE_EMISSIVE, 0), -1)
    return f.reshape(h, w)


def make_orbit_golden(path):
    """Writes the fixture ORBIT_GOLDEN: two minutes of the oracle's per-pixel loop (view_ref.render), so it is
    computed once and committed instead of in every test run.  `python tests/temporal_ref.py PATH`."""
    import conftest
    import oracle
    import view_ref
    osc = oracle.OracleScene(conftest.load_scene("cornell").arrays())
    pos, view = orbit_pose(ORBIT_FRAMES - 1)
    img = view_ref.render(osc, (pos, 1.0, 3.0, 0.0, ORBIT_SIZE, ORBIT_SIZE), view, ORBIT_REF_SPP, 3, 0, ORBIT_SEED + 1000)
    np.save(path, img.astype(F))


class TemporalRef:
    def __init__(self, width, height, max_history=32, normal_min=0.9, plane_tol=0.02):
        self.w, self.h = int(width), int(height)
        self.max_history, self.normal_min, self.plane_tol = F(int(max_history)), F(normal_min), F(plane_tol)
        self.reset()

    def reset(self):
        self.frames = 0
        self.prev = None          # (cam, view, off) of the previous push
        self.P = self.N = self.prim = self.C = self.n = self.m1 = self.m2 = None
        self.stats = {}

    def history_length(self):
        return np.zeros((self.h, self.w), dtype=F) if self.n is None else self.n.copy()

    def push(self, img, feat, cam, view=None, flags=0):
        H, W = self.h, self.w
        assert cam[4] == W and cam[5] == H
        inp = np.ascontiguousarray(img, dtype=F).reshape(H, W, 3)
        feat = np.asarray(feat).reshape(H, W)
        P = np.ascontiguousarray(feat["position"], dtype=F)
        N = np.ascontiguousarray(feat["normal"], dtype=F)
        prim = np.ascontiguousarray(feat["prim"], dtype=np.int32)
        depth = np.ascontiguousarray(feat["depth"], dtype=F)
        zero = np.zeros((H, W), dtype=F)
        ws, hn, h1, h2 = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        hc = np.zeros((H, W, 3), dtype=F)
        st = dict(first=self.frames == 0, miss=int(np.count_nonzero(prim < 0)))
        if self.frames == 0:
            reset = np.ones((H, W), dtype=bool)
        else:
            pcam, pview, off = self.prev
            front, sx, sy = project(pcam, pview, P)
            hit = prim >= 0
            reset = ~hit | ~front
            with np.errstate(all="ignore"):
                fx = sx - off
                fy = sy - off
            exact = hit & front & (fx == np.floor(fx)) & (fy == np.floor(fy))
            with np.errstate(all="ignore"):
                near_miss = hit & front & (np.abs(fx - np.floor(fx + F(0.5))) > SNAP) & (np.abs(fx - np.floor(fx + F(0.5))) <= F(2) * SNAP)
            fx, nx = _snap(fx)
            fy, ny = _snap(fy)
            with np.errstate(invalid="ignore"):
                inx = (fx > F(-1)) & (fx < F(W))
                iny = (fy > F(-1)) & (fy < F(H))
            seen = hit & front
            st.update(behind=int(np.count_nonzero(hit & ~front)), left=int(np.count_nonzero(seen & ~(fx > F(-1)))),
                      right=int(np.count_nonzero(seen & ~(fx < F(W)))), top=int(np.count_nonzero(seen & ~(fy > F(-1)))),
                      bottom=int(np.count_nonzero(seen & ~(fy < F(H)))), exact=int(np.count_nonzero(exact)),
                      snapped=int(np.count_nonzero(seen & nx & ny & ~exact)), just_beyond_snap=int(np.count_nonzero(near_miss)))
            reset = reset | ~inx | ~iny
            fx = np.where(reset, F(0), fx).astype(F)
            fy = np.where(reset, F(0), fy).astype(F)
            x0 = np.floor(fx).astype(np.int64)
            y0 = np.floor(fy).astype(np.int64)
            tx = fx - x0.astype(F)
            ty = fy - y0.astype(F)
            st.update(x0_minus1=int(np.count_nonzero(~reset & (x0 == -1))), x0_last=int(np.count_nonzero(~reset & (x0 == W - 1))),
                      y0_minus1=int(np.count_nonzero(~reset & (y0 == -1))), y0_last=int(np.count_nonzero(~reset & (y0 == H - 1))),
                      fractional=int(np.count_nonzero(~reset & (tx > 0) & (ty > 0))))
            lim = self.plane_tol * depth
            cat = dict(tap_outside=0, tap_miss=0, tap_empty=0, tap_normal_only=0, tap_plane_only=0, tap_both_fail=0, tap_pass=0)
            for t in range(4):
                xq = x0 + (t & 1)
                yq = y0 + (t >> 1)
                wx = tx if (t & 1) else F(1) - tx
                wy = ty if (t >> 1) else F(1) - ty
                w = wx * wy
                inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                Pq, Nq, primq = self.P[yc, xc], self.N[yc, xc], self.prim[yc, xc]
                Cq, nq, m1q, m2q = self.C[yc, xc], self.n[yc, xc], self.m1[yc, xc], self.m2[yc, xc]
                a = N[..., 0] * Nq[..., 0]
                b = N[..., 1] * Nq[..., 1]
                a = a + b
                b = N[..., 2] * Nq[..., 2]
                dn = a + b
                a = N[..., 0] * (Pq[..., 0] - P[..., 0])
                b = N[..., 1] * (Pq[..., 1] - P[..., 1])
                a = a + b
                b = N[..., 2] * (Pq[..., 2] - P[..., 2])
                e = np.abs(a + b)
                live = ~reset & inside
                holds = live & (primq >= 0) & (nq > F(0))
                n_ok, p_ok = dn >= self.normal_min, e <= lim
                ok = holds & n_ok & p_ok
                cat["tap_outside"] += int(np.count_nonzero(~reset & ~inside))
                cat["tap_miss"] += int(np.count_nonzero(live & (primq < 0)))
                cat["tap_empty"] += int(np.count_nonzero(live & (primq >= 0) & ~(nq > F(0))))
                cat["tap_normal_only"] += int(np.count_nonzero(holds & ~n_ok & p_ok))
                cat["tap_plane_only"] += int(np.count_nonzero(holds & n_ok & ~p_ok))
                cat["tap_both_fail"] += int(np.count_nonzero(holds & ~n_ok & ~p_ok))
                cat["tap_pass"] += int(np.count_nonzero(ok))
                ws = np.where(ok, ws + w, ws)
                for k in range(3):
                    hc[..., k] = np.where(ok, hc[..., k] + w * Cq[..., k], hc[..., k])
                hn = np.where(ok, hn + w * nq, hn)
                h1 = np.where(ok, h1 + w * m1q, h1)
                h2 = np.where(ok, h2 + w * m2q, h2)
            st.update(cat)
        use = (ws > F(0)) & ~reset
        with np.errstate(all="ignore"):
            for k in range(3):
                hc[..., k] = np.where(use, hc[..., k] / ws, F(0))
            hn = np.where(use, hn / ws, F(0)).astype(F)
            h1 = np.where(use, h1 / ws, F(0)).astype(F)
            h2 = np.where(use, h2 / ws, F(0)).astype(F)
        n1 = hn + F(1)
        n1 = np.where(n1 < self.max_history, n1, self.max_history).astype(F)
        al = F(1) / n1
        out = np.empty((H, W, 3), dtype=F)
        for k in range(3):
            d = inp[..., k] - hc[..., k]
            d = d * al
            out[..., k] = hc[..., k] + d
        l = lum(inp)
        d = l - h1
        d = d * al
        m1 = h1 + d
        d = l * l
        d = d - h2
        d = d * al
        m2 = h2 + d
        d = m1 * m1
        d = m2 - d
        d = np.where(d > F(0), d, F(0)).astype(F)
        with np.errstate(all="ignore"):
            v = d / (n1 - F(1))
        var = np.where(n1 < F(2), F(np.inf), v).astype(F)
        for a in (out, n1, m1, m2, var):
            assert a.dtype == F
        st.update(history_used=int(np.count_nonzero(use)), n_max=float(n1.max()), n_at_cap=int(np.count_nonzero(n1 == self.max_history)))
        self.stats = st
        self.P, self.N, self.prim = P.copy(), N.copy(), prim.copy()
        self.C, self.n, self.m1, self.m2 = out.copy(), n1, m1, m2
        self.prev = (cam, view, F(0.5) if (flags & PT_FLAG_JITTER) else F(0.0))
        self.frames += 1
        return out, var


if __name__ == "__main__":
    import sys
    make_orbit_golden(sys.argv[1])
