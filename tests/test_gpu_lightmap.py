"""Lightmap finishing on the GPU (include/pt/pt.h, pt_lightmap_*): the gutter fill and the lightmapped view equal their
numpy restatements (lightmap_ref.py) in every bit; what they refuse; the seam a dilation removes, end to end over a
bake; and nothing of either call stays behind in the context.  Nothing here has a tolerance."""
import os

import numpy as np
import pytest
import torch

from conftest import MODELS, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import rays

import lightmap_ref as lr

pytestmark = pytest.mark.gpu

F = np.float32
POS = (0.0, 1.0, 3.0)
SIZES = [(1, 1), (3, 100), (100, 3), (37, 19), (64, 64), (130, 70)]   # the tile is 64 x 32
RADII = [0, 1, 2, 7, 16]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cam(w, h):
    return pt.make_camera(POS, 1.0, 3.0, 0.0, w, h)


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def renderer(scene):
    assert hasattr(pt.Renderer, "lightmap_dilate")
    r = pt.Renderer(scene, 0)
    yield r
    r.close()


# ---- a. the gutter fill
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_dilate_equals_the_restatement(renderer, size, radius):
    W, H = size
    img = lr.odd_image(W, H, 17 * W + H)
    d_img = _dev(img)
    for name, mask in lr.masks(W, H, radius, 1000 * radius + W).items():
        want, want_src = lr.dilate(img, mask, radius)
        if name == "one":     # exactly `radius` away diagonally it is found, one texel farther it is not
            if W > radius and H > radius and radius > 0:
                assert want_src[H - 1 - radius, W - 1 - radius] == W * H - 1
            if W > radius + 1 and H > radius + 1:
                assert want_src[H - 2 - radius, W - 2 - radius] == -1
        if name == "column0" and W > radius + 1:
            assert (want_src[:, W - 1] == -1).all()        # no wrap-around
        d_mask = _dev(mask)
        d_out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        d_src = torch.full((H, W), -9, dtype=torch.int32, device="cuda")
        renderer.lightmap_dilate_device(d_img.data_ptr(), d_mask.data_ptr(), d_out.data_ptr(), W, H, radius, d_src.data_ptr())
        assert d_out.cpu().numpy().tobytes() == want.tobytes(), (name, "out")
        assert (d_src.cpu().numpy() == want_src).all(), (name, "src")
        # in place, without src
        d_io = d_img.clone()
        renderer.lightmap_dilate_device(d_io.data_ptr(), d_mask.data_ptr(), d_io.data_ptr(), W, H, radius)
        assert d_io.cpu().numpy().tobytes() == want.tobytes(), (name, "in place")
        if name in ("half", "corners"):                      # the host variant
            out, src = renderer.lightmap_dilate(img, mask, radius, return_src=True)
            assert out.tobytes() == want.tobytes() and (src == want_src).all(), (name, "host")
            assert renderer.lightmap_dilate(img, mask, radius).tobytes() == want.tobytes()
    assert d_img.cpu().numpy().tobytes() == img.tobytes()     # the input is read only


def test_dilate_cases_are_not_vacuous():
    """At 64 x 64 the lone covered texel is found at every radius and missed one texel farther; the checkerboard makes
    both kinds of tie."""
    for radius in RADII[1:]:
        _, src = lr.dilate(lr.odd_image(64, 64, 1), lr.masks(64, 64, radius, 1)["one"], radius)
        assert src[63 - radius, 63 - radius] == 64 * 64 - 1 and src[62 - radius, 62 - radius] == -1
    _, src = lr.dilate(lr.odd_image(8, 8, 1), lr.masks(8, 8, 1, 1)["checker"], 1)
    assert src[2, 2] == 1 * 8 + 2                              # up, down, left and right tie: up


# ---- b. the lightmapped view
@pytest.fixture(scope="module")
def shade_scenes(scene, tmp_path_factory):
    """name -> (scene, renderer): the Cornell box; with a diffuse and an emissive sphere; with a degenerate triangle
    appended (two of its corners coincide, so no ray hits it and det is 0 for it)."""
    out = {}
    s = load_scene("cornell")
    s.add_sphere((0.4, 0.3, 0.5), 0.3, (0.6, 0.7, 0.8))
    s.add_sphere((-0.5, 0.25, 0.6), 0.25, (0.5, 0.5, 0.5), (3.0, 3.0, 3.0))
    out["spheres"] = s
    d = tmp_path_factory.mktemp("lightmap")
    txt = open(os.path.join(MODELS, "cornell.obj")).read() + "\no degenerate\nv 0.25 0.5 0.25\nv 0.5 0.5 0.25\nf -2 -2 -1\n"
    with open(os.path.join(str(d), "degenerate.obj"), "w") as f:
        f.write(txt)
    s = pt.Scene()
    s.load_obj(os.path.join(str(d), "degenerate.obj"), (0, 0, 0), 1.0, mtl_basepath=MODELS + "/")
    s.build_bvh()
    out["degenerate"] = s
    out["cornell"] = scene
    rs = {k: (v, pt.Renderer(v, 0)) for k, v in out.items()}
    yield rs
    for _, r in rs.values():
        r.close()


def _feature_sets(r, w, h):
    cam = _cam(w, h)
    view = pt.look_at((1.6, 1.4, 3.2), (-0.3, 0.6, -0.2), cam=cam, vfov=50.0)
    o, d = rays.ortho_rays(POS, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 3.0, 3.0, w, h)
    return {"camera": r.features(cam, w, h), "look_at": r.features(cam, w, h, view=view),
            "ortho": r.features_rays(o, d, w, h)}


@pytest.mark.parametrize("size", [(24, 16), (37, 19)], ids=lambda s: "%dx%d" % s)
def test_shade_equals_the_restatement(shade_scenes, size):
    w, h = size
    rng = np.random.RandomState(w)
    maps = [rng.rand(16, 16, 3).astype(F) * 4, rng.rand(3, 5, 3).astype(F), rng.rand(1, 1, 3).astype(F)]
    seen = set()
    calls = 0
    for sname, (s, r) in shade_scenes.items():
        arrays = s.arrays()
        nt = arrays["tris"].shape[0]
        tris, uvs, floor = lr.cornell_chart(arrays)
        table = rays.chart_uv_table(nt, tris, uvs)
        assert np.isnan(table[:, 0]).sum() == nt - len(tris) > 0
        assert (table[tris[len(floor):]] == 0).any() and (table[tris[len(floor):]] == 1).any()    # the edge clamps fire
        if sname == "degenerate":
            table[nt - 1] = (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)       # (charted, so that its det decides)
        tables = {"chart": table}
        t = table.copy()
        t[tris[-1], 2] = np.inf                                  # a chart coordinate that is not finite: s is not
        tables["inf"] = t
        t = table.copy()
        t[tris[-1]] = np.tile(t[tris[-1], :2], 3)                # a degenerate chart triangle: one point of the map
        tables["point"] = t
        for fname, feat in _feature_sets(r, w, h).items():
            if sname == "degenerate":                            # no ray finds that triangle: name it by hand
                feat = feat.copy()
                feat.reshape(-1)["prim"][:3] = nt - 1
            for tname, tab in tables.items():
                for k, lm in enumerate(maps):
                    fill, flags = ((0.0, 0.0, 0.0), 0) if k == 0 else ((0.25, -2.0, 7.5), k & 1)
                    want, cls = lr.shade(feat, tab, lm, arrays, fill, flags)
                    got = r.lightmap_shade(feat, tab, lm, fill, flags)
                    assert got.shape == feat.shape + (3,)
                    assert got.tobytes() == want.tobytes(), (sname, fname, tname, k)
                    seen |= set(np.unique(cls).tolist())
                    calls += 1
        # the device variant, once per scene; and no record at all
        feat = r.features(_cam(w, h), w, h)
        want, _ = lr.shade(feat, table, maps[0], arrays, (1.0, 2.0, 3.0), lr.NO_ALBEDO)
        d_feat, d_tab, d_map = _dev(feat.view(np.uint8)), _dev(table), _dev(maps[0])
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        r.lightmap_shade_device(d_feat.data_ptr(), w * h, d_tab.data_ptr(), d_map.data_ptr(), 16, 16, d_out.data_ptr(),
                                (1.0, 2.0, 3.0), lr.NO_ALBEDO)
        assert d_out.cpu().numpy().tobytes() == want.tobytes()
        d_out.fill_(-7.0)
        r.lightmap_shade_device(d_feat.data_ptr(), 0, d_tab.data_ptr(), d_map.data_ptr(), 16, 16, d_out.data_ptr())
        assert (d_out.cpu().numpy() == -7.0).all()
        assert r.lightmap_shade(np.zeros(0, pt.FEATURE), table, maps[0]).shape == (0, 3)
    assert calls == 3 * 3 * 3 * 3
    # every way to `fill` occurred, and so did a looked-up value: the case data is not vacuous
    assert seen == set(lr.FILL_CLASSES) | {lr.SHADED}, seen


# ---- c. refusals
def _refused(call, word):
    with pytest.raises(pt.PtError) as e:
        call()
    assert e.value.code == pt.PT_E_INVALID and word in str(e.value), str(e.value)


def test_refusals_leave_the_output_untouched(renderer, scene):
    r = renderer
    W, H = 20, 12
    d_img, d_mask = _dev(lr.odd_image(W, H, 1)), _dev(lr.masks(W, H, 1, 1)["half"])
    d_out = torch.full((H * W * 3 + 4,), -7.0, dtype=torch.float32, device="cuda")
    d_src = torch.full((H * W + 4,), -9, dtype=torch.int32, device="cuda")
    i, m, o, s = d_img.data_ptr(), d_mask.data_ptr(), d_out.data_ptr(), d_src.data_ptr()
    _refused(lambda: r.lightmap_dilate_device(i, m, o, W, H, 17, s), "radius")
    _refused(lambda: r.lightmap_dilate_device(i, m, o, W, H, -1, s), "radius")
    _refused(lambda: r.lightmap_dilate_device(i, m, o, 0, H, 1, s), "width")
    _refused(lambda: r.lightmap_dilate_device(i, m, o, W, 65536, 1, s), "height")
    _refused(lambda: r.lightmap_dilate_device(0, m, o, W, H, 1, s), "null d_in")
    _refused(lambda: r.lightmap_dilate_device(i, 0, o, W, H, 1, s), "null d_covered")
    _refused(lambda: r.lightmap_dilate_device(i, m, 0, W, H, 1, s), "null d_out")
    _refused(lambda: r.lightmap_dilate_device(i + 2, m, o, W, H, 1, s), "d_in is not 4-byte aligned")
    _refused(lambda: r.lightmap_dilate_device(i, m, o + 1, W, H, 1, s), "d_out is not 4-byte aligned")
    _refused(lambda: r.lightmap_dilate_device(i, m, o, W, H, 1, s + 2), "d_src is not 4-byte aligned")
    _refused(lambda: r.lightmap_dilate(np.zeros((H, W, 3), F), np.ones((H, W)), 17), "radius")

    nt = scene.arrays()["tris"].shape[0]
    feat = r.features(_cam(W, H), W, H)
    d_feat = _dev(np.concatenate([feat.reshape(-1), np.zeros(1, pt.FEATURE)]).view(np.uint8))
    d_tab, d_map = _dev(np.zeros((nt, 6), F)), _dev(np.ones((4, 4, 3), F))
    f, t, p, n = d_feat.data_ptr(), d_tab.data_ptr(), d_map.data_ptr(), W * H
    _refused(lambda: r.lightmap_shade_device(f, n, t, p, 4, 4, o, flags=2), "flags")
    _refused(lambda: r.lightmap_shade_device(f, n, t, p, 0, 4, o), "map_w")
    _refused(lambda: r.lightmap_shade_device(f, n, t, p, 4, 65536, o), "map_h")
    _refused(lambda: r.lightmap_shade_device(0, n, t, p, 4, 4, o), "null d_feat")
    _refused(lambda: r.lightmap_shade_device(f, n, 0, p, 4, 4, o), "null d_tri_uv")
    _refused(lambda: r.lightmap_shade_device(f, n, t, 0, 4, 4, o), "null d_map")
    _refused(lambda: r.lightmap_shade_device(f, n, t, p, 4, 4, 0), "null d_out")
    _refused(lambda: r.lightmap_shade_device(f + 8, n, t, p, 4, 4, o), "d_feat is not 16-byte aligned")
    _refused(lambda: r.lightmap_shade_device(f, n, t + 2, p, 4, 4, o), "d_tri_uv is not 4-byte aligned")
    _refused(lambda: r.lightmap_shade_device(f, n, t, p + 1, 4, 4, o), "d_map is not 4-byte aligned")
    _refused(lambda: r.lightmap_shade_device(f, n, t, p, 4, 4, o + 2), "d_out is not 4-byte aligned")
    _refused(lambda: r.lightmap_shade(feat, np.zeros((nt, 6), F), np.ones((4, 4, 3), F), flags=4), "flags")
    with pytest.raises(ValueError):
        r.lightmap_shade(feat, np.zeros((nt + 1, 6), F), np.ones((4, 4, 3), F))

    # while a render is in flight
    d_frame = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    r.render_device_async(_cam(W, H), d_frame.data_ptr(), W, H, 2)
    try:
        _refused(lambda: r.lightmap_dilate_device(i, m, o, W, H, 1, s), "in flight")
        _refused(lambda: r.lightmap_shade_device(f, n, t, p, 4, 4, o), "in flight")
        _refused(lambda: r.lightmap_dilate(np.zeros((H, W, 3), F), np.ones((H, W)), 1), "in flight")
        _refused(lambda: r.lightmap_shade(feat, np.zeros((nt, 6), F), np.ones((4, 4, 3), F)), "in flight")
    finally:
        r.wait()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all() and (d_src.cpu().numpy() == -9).all()
    # and the same calls go through afterwards
    r.lightmap_dilate_device(i, m, o, W, H, 1, s)
    r.lightmap_shade_device(f, n, t, p, 4, 4, o)


# ---- d. the seam, end to end
def test_dilation_removes_the_seam(renderer, scene):
    r = renderer
    arrays = scene.arrays()
    nt = arrays["tris"].shape[0]
    tris, uvs, floor = lr.cornell_chart(arrays, 0.1, 0.9)
    tris, uvs = tris[:len(floor)], uvs[:len(floor)]              # the floor alone, on [0.1, 0.9]^2 of 16 x 16 texels
    M = 16
    p, n, tri, covered = rays.chart_points(arrays, tris, uvs, M, M)
    cov = covered.reshape(M, M)
    want_cov = np.zeros((M, M), bool)
    want_cov[2:14, 2:14] = True
    assert (cov == want_cov).all()
    table = rays.chart_uv_table(nt, tris, uvs)
    w, h = 48, 32
    feat = r.features(_cam(w, h), w, h)
    on_floor = np.isin(feat["prim"], floor)
    assert on_floor.sum() > 100
    albedo = feat["albedo"][on_floor]
    assert (albedo > 0).all()

    # 1.0 on the covered texels, 0 elsewhere
    lm = np.where(cov[..., None], F(1.0), F(0.0)).astype(F) * np.ones(3, F)
    raw = r.lightmap_shade(feat, table, lm)[on_floor]
    assert (raw <= albedo).all() and (raw < albedo).any()         # the seam: floor pixels below their albedo
    filled, src = r.lightmap_dilate(lm, cov, 1, return_src=True)
    assert (filled[1:15, 1:15] == 1.0).all() and (src[0] == -1).all()
    seamless = r.lightmap_shade(feat, table, filled)[on_floor]
    assert seamless.tobytes() == albedo.tobytes()                 # every charted floor pixel equals its albedo exactly

    # the same over a real bake of that chart
    with r.accumulator_points(p, n, M, M, 3, 0, 1234) as acc:
        acc.freeze(~cov)
        acc.add(4)
        bake = acc.image()
    assert (bake[~cov] == 0).all() and (bake[cov] > 0).any() and (bake >= 0).all()
    baked = r.lightmap_dilate(bake, cov, 1)
    a, b = r.lightmap_shade(feat, table, bake)[on_floor], r.lightmap_shade(feat, table, baked)[on_floor]
    # the pixels whose weighted taps include an uncovered texel: where the covered flags themselves do not look up as 1
    flags_view, _ = lr.shade(feat, table, lm, arrays, flags=lr.NO_ALBEDO)
    touched = (flags_view[on_floor] != 1.0).any(axis=1)
    assert 0 < touched.sum() < touched.size
    assert a[~touched].tobytes() == b[~touched].tobytes()
    assert (b[touched] >= a[touched]).all() and (b[touched] > a[touched]).any()
    assert (a != b).any(axis=1)[touched].sum() > 0


# ---- e. everything else is untouched
def test_nothing_stays_behind_in_the_context(renderer, scene):
    r = renderer
    w, h = 24, 16
    cam = _cam(w, h)
    before = [r.render(cam, w, h, 2, 3, integ, 1234)[0].tobytes() for integ in (0, 1)]
    feat = r.features(cam, w, h)
    arrays = scene.arrays()
    tris, uvs, _ = lr.cornell_chart(arrays)
    table = rays.chart_uv_table(arrays["tris"].shape[0], tris, uvs)
    lm = lr.odd_image(16, 16, 5)
    filled = r.lightmap_dilate(lm, lr.masks(16, 16, 4, 5)["half"], 4)
    r.lightmap_shade(feat, table, filled)
    after = [r.render(cam, w, h, 2, 3, integ, 1234)[0].tobytes() for integ in (0, 1)]
    assert before == after
    assert r.features(cam, w, h).tobytes() == feat.tobytes()
