"""Lightmap finishing without a GPU (include/pt/pt.h, pt_lightmap_*): the numpy restatement of both rules
(lightmap_ref.py) against hand-worked cases, the layouts of rays.chart_uv_table and rays.point_features, the exported
symbols, and the refusals that need no device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, rays

import lightmap_ref as lr

F = np.float32


def _mask(points, W=8, H=8):
    m = np.zeros((H, W), np.uint8)
    for x, y in points:
        m[y, x] = 1
    return m


def _img(W=8, H=8):
    """Texel (x, y) holds (100*y + x, its negative, NaN with the index as payload)."""
    ys, xs = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), F)
    img[..., 0] = 100 * ys + xs
    img[..., 1] = -img[..., 0]
    img.view(np.uint32)[..., 2] = 0x7fc00000 + (W * ys + xs).astype(np.uint32)
    return img


def test_dilate_restatement_on_hand_worked_ties():
    img = _img()
    # a tie in i: (2,3) and (4,3) are both 1 away from (3,3); the smaller i, the left one, wins
    out, src = lr.dilate(img, _mask([(2, 3), (4, 3)]), 1)
    assert src[3, 3] == 3 * 8 + 2 and out[3, 3, 0] == 302.0
    assert out.view(np.uint32)[3, 3, 2] == 0x7fc00000 + 26              # the NaN's payload came along
    # a tie in j: (3,1) above and (3,3) below (3,2); the smaller j, the upper one, wins
    out, src = lr.dilate(img, _mask([(3, 1), (3, 3)]), 1)
    assert src[2, 3] == 1 * 8 + 3 and out[2, 3, 1] == -103.0
    # equal distances in different rows: j decides before i -- (i=0, j=-1) beats (i=-1, j=0) and (i=+1, j=0) ...
    out, src = lr.dilate(img, _mask([(2, 3), (4, 3), (3, 2)]), 2)
    assert src[3, 3] == 2 * 8 + 3
    # ... and (i=+1, j=0) beats (i=0, j=+1)
    out, src = lr.dilate(img, _mask([(4, 3), (3, 4)]), 2)
    assert src[3, 3] == 3 * 8 + 4
    # (i=-1, j=-2) and (i=2, j=1) are both 5 away: the smaller j
    out, src = lr.dilate(img, _mask([(2, 1), (5, 4)]), 3)
    assert src[3, 3] == 1 * 8 + 2
    # the window is a square: (0,0) is 3 away from (3,3) in both axes, inside radius 3, outside radius 2
    m = _mask([(0, 0)])
    assert lr.dilate(img, m, 3)[1][3, 3] == 0 and lr.dilate(img, m, 2)[1][3, 3] == -1
    # covered texels keep theirs, nothing in reach keeps its own with src -1, radius 0 is a copy, no wrap-around
    out, src = lr.dilate(img, m, 2)
    assert src[0, 0] == 0 and src[7, 7] == -1 and out.tobytes()[-12:] == img.tobytes()[-12:]
    out, src = lr.dilate(img, _mask([(2, 3)]), 0)
    assert out.tobytes() == img.tobytes() and src[3, 2] == 26 and (np.delete(src.reshape(-1), 26) == -1).all()
    out, src = lr.dilate(img, _mask([(7, 2)]), 1)
    assert src[2, 0] == -1 and src[3, 0] == -1 and src[2, 6] == 23
    # the vectorised scan is the tap-by-tap one
    rng = np.random.RandomState(7)
    for W, H, r in ((8, 8, 2), (5, 7, 3), (9, 4, 16), (1, 1, 1), (3, 20, 7)):
        odd = lr.odd_image(W, H, 3)
        for name, m in lr.masks(W, H, r, rng.randint(1 << 30)).items():
            a, b = lr.dilate(odd, m, r), lr.dilate_scalar(odd, m, r)
            assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all(), (W, H, r, name)


@pytest.fixture(scope="module")
def arrays():
    return load_scene("cornell").arrays()


def _floor_features(arrays, floor, n, seed):
    """n records on the first floor triangle at random barycentrics, albedo random."""
    rng = np.random.RandomState(seed)
    b1 = rng.rand(n)
    b2 = rng.rand(n) * (1 - b1)
    p, nrm = rays.triangle_points(arrays, np.full(n, floor[0]), b1, b2, lift=0.0)
    f = rays.point_features(p, nrm, np.full(n, floor[0]))
    f["albedo"] = rng.rand(n, 3).astype(F)
    return f


def test_shade_restatement_on_hand_worked_cases(arrays):
    tris, uvs, floor = lr.cornell_chart(arrays)
    table = rays.chart_uv_table(arrays["tris"].shape[0], tris, uvs)
    f = _floor_features(arrays, floor, 64, 11)
    # a constant map comes back exactly, times the albedo
    const = np.empty((5, 7, 3), F)
    const[:] = (0.3, 1.7, 123.456)
    out, cls = lr.shade(f, table, const, arrays)
    assert (cls == lr.SHADED).all()
    assert out.tobytes() == (f["albedo"] * const[0, 0]).astype(F).tobytes()
    out, _ = lr.shade(f, table, const, arrays, flags=lr.NO_ALBEDO)
    assert out.tobytes() == np.broadcast_to(const[0, 0], (64, 3)).astype(F).tobytes()
    # a 2 x 1 map holding 0 and 1 reads back the horizontal position: the floor's chart spans [0.1, 0.9], so
    # s = 2u - 0.5 runs from -0.3 (clamped to the left texel) to 1.3 (the right one)
    ramp = np.zeros((1, 2, 3), F)
    ramp[0, 1] = 1.0
    out, _ = lr.shade(f, table, ramp, arrays, flags=lr.NO_ALBEDO)
    x = f["position"][:, 0].astype(np.float64)            # the floor spans x in [-1, 1] and u = 0.5 + 0.4 x
    want = np.clip(2 * (0.5 + 0.4 * x) - 0.5, 0.0, 1.0)
    assert np.abs(out[:, 0] - want).max() < 1e-5
    # the classes: a miss, an emitter, a sphere id, a triangle of no chart, a non-finite chart coordinate
    g = f[:5].copy()
    g["prim"] = [-1, floor[0] | lr.PT_FEATURE_EMISSIVE, arrays["tris"].shape[0], 0, floor[0]]
    t2 = table.copy()
    no_chart = int(np.flatnonzero(np.isnan(table[:, 0]))[0])
    g["prim"][3] = no_chart
    out, cls = lr.shade(g, t2, const, arrays, fill=(9, 8, 7))
    assert list(cls) == [lr.MISS, lr.EMISSIVE, lr.SPHERE, lr.NO_CHART, lr.SHADED]
    assert (out[:4] == np.array([9, 8, 7], F)).all() and (out[4] != np.array([9, 8, 7], F)).all()
    t2[floor[0], 2] = np.inf
    assert lr.shade(g, t2, const, arrays)[1][4] == lr.ST


def test_chart_uv_table_layout(arrays):
    nt = arrays["tris"].shape[0]
    tris, uvs, floor = lr.cornell_chart(arrays)
    table = rays.chart_uv_table(nt, tris, uvs)
    assert table.shape == (nt, 6) and table.dtype == F
    for k, t in enumerate(tris):
        assert table[t].tobytes() == uvs[k].reshape(6).astype(F).tobytes()
    rest = np.setdiff1d(np.arange(nt), tris)
    assert rest.size and np.isnan(table[rest]).all()
    # the first entry of a triangle listed twice holds, as in chart_points
    twice = rays.chart_uv_table(nt, [3, 3], np.stack([uvs[0], uvs[1]]))
    assert twice[3].tobytes() == uvs[0].reshape(6).astype(F).tobytes()
    assert np.isnan(rays.chart_uv_table(4, [], np.zeros((0, 3, 2)))).all()
    with pytest.raises(ValueError):
        rays.chart_uv_table(nt, [nt], uvs[:1])
    with pytest.raises(ValueError):
        rays.chart_uv_table(nt, [0], uvs[:2])


def test_point_features_layout(arrays):
    tris, uvs, floor = lr.cornell_chart(arrays)
    p, n, tri, covered = rays.chart_points(arrays, tris[:2], uvs[:2], 16, 16)
    assert covered.reshape(16, 16)[2:14, 2:14].all() and covered.sum() == 144     # texels 2..13 of [0.1, 0.9]^2
    f = rays.point_features(p, n, tri)
    assert f.dtype == pt.FEATURE and f.shape == (256,)
    assert (f["albedo"] == 1).all() and (f["depth"] == 1).all() and (f["reserved"] == 0).all()
    assert f["position"].tobytes() == p.tobytes() and f["normal"].tobytes() == n.tobytes()
    assert (f["prim"][covered] == tri[covered]).all() and (f["prim"][~covered] == -1).all()
    assert rays.point_features(p, n, tri.reshape(16, 16)).shape == (16, 16)
    with pytest.raises(ValueError):
        rays.point_features(p[:5], n, tri)


def test_exported_symbols_and_constants():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pt_lightmap_[a-z0-9_]+)", out))
    assert exported == {"pt_lightmap_dilate", "pt_lightmap_dilate_device", "pt_lightmap_shade", "pt_lightmap_shade_device"}
    assert exported <= set(_lib.SIGNATURES)
    assert C.sizeof(_lib.LightmapParams) == 16 and pt.PT_LIGHTMAP_NO_ALBEDO == 1
    assert _lib.lib().pt_abi_version() == 6


def _refused(rc, word):
    assert rc == _lib.PT_E_INVALID
    msg = _lib.lib().pt_last_error().decode()
    assert word in msg, msg


def test_refusals_that_need_no_device():
    L = _lib.lib()
    img = np.zeros((4, 4, 3), F)
    cov = np.ones((4, 4), np.uint8)
    out = np.full((4, 4, 3), -7.0, F)
    i, c, o = img.ctypes.data, cov.ctypes.data, out.ctypes.data
    for fn, extra, d in ((L.pt_lightmap_dilate, (), ""), (L.pt_lightmap_dilate_device, (None,), "d_")):
        _refused(fn(None, 4, 4, 17, i, c, o, None, *extra), "radius")
        _refused(fn(None, 4, 4, -1, i, c, o, None, *extra), "radius")
        _refused(fn(None, 0, 4, 1, i, c, o, None, *extra), "width")
        _refused(fn(None, 4, -3, 1, i, c, o, None, *extra), "height")
        _refused(fn(None, 65535, 65535, 1, i, c, o, None, *extra), "texels")
        _refused(fn(None, 4, 4, 1, None, c, o, None, *extra), "null %sin" % d)
        _refused(fn(None, 4, 4, 1, i, None, o, None, *extra), "null %scovered" % d)
        _refused(fn(None, 4, 4, 1, i, c, None, None, *extra), "null %sout" % d)
        _refused(fn(None, 4, 4, 1, i, c, o, None, *extra), "null ctx")
    lp = _lib.LightmapParams()
    feat = np.zeros(4, pt.FEATURE)
    uv = np.zeros((2, 6), F)
    f, u = feat.ctypes.data, uv.ctypes.data
    for fn, extra, d in ((L.pt_lightmap_shade, (), ""), (L.pt_lightmap_shade_device, (None,), "d_")):
        _refused(fn(None, None, 4, f, u, i, 4, 4, o, *extra), "params")
        lp.flags = 2
        _refused(fn(None, C.byref(lp), 4, f, u, i, 4, 4, o, *extra), "flags")
        lp.flags = 1
        _refused(fn(None, C.byref(lp), 4, f, u, i, 0, 4, o, *extra), "map_w")
        _refused(fn(None, C.byref(lp), 4, f, u, i, 4, 70000, o, *extra), "map_h")
        _refused(fn(None, C.byref(lp), 4, f, u, None, 4, 4, o, *extra), "null %smap" % d)
        _refused(fn(None, C.byref(lp), 4, f, u, i, 4, 4, o, *extra), "null ctx")
    assert (out == -7.0).all()
