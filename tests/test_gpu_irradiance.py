"""Irradiance renders on the GPU (include/pt/pt.h, pt_render_irradiance*, pt_points_classify_device): every image equals
irradiance_ref -- the definition's per-pixel loop around the oracle's integrators, a cosine-weighted direction per
sample -- in every bit, on the wavefront kernels (both integrators, split units, the flags), on the tile kernel (the
reference flags, PT_HEAD_WF=0, an irregular buffer) and through every shard / tile / order geometry; the classification
kernel equals its numpy restatement.  Cornell box, 24 x 16, 4 samples, 3 bounces, seed 1234 unless said otherwise."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import MODELS, ROOT, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import rays, scenes, shard
from cudapathtracer_amd.rays import feature_points, grid_points                    # (the parent has none: every test here errors there)
import irradiance_ref as iref
import light_scenes as ls
import oracle

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, SPP, BOUNCES, SEED = 24, 16, 4, 3, 1234
POS = iref.POS
RT, RB, NPC, NDPS = (pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH, pt.PT_FLAG_NO_PRIMARY_CACHE,
                     pt.PT_FLAG_NO_DEAD_PATH_SKIP)
SENTINEL = -7.0


def _renderer(scene, env):
    """A renderer created with `env` set: the PT_* knobs are read at pt_create."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pt.Renderer(scene, 0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def osc(scene):
    return oracle.OracleScene(scene.arrays())


@pytest.fixture(scope="module")
def renderers(scene):
    rs = {"default": _renderer(scene, {}), "tile_head": _renderer(scene, {"PT_HEAD_WF": "0"}),
          "chunks": _renderer(scene, {"PT_WF_CHUNKS": "3"}), "whole": _renderer(scene, {"PT_WF_CHUNKS": "1"})}
    yield rs
    for r in rs.values():
        r.close()


@pytest.fixture(scope="module")
def blob():
    """Cornell box + blob: the scene of set b, with its renderer and its oracle scene."""
    s = load_scene("cornell_blob")
    r = pt.Renderer(s, 0)
    yield s, r, oracle.OracleScene(s.arrays())
    r.close()


def _cam(w=W, h=H):
    return pt.make_camera(POS, 1.0, 3.0, 0.0, w, h)


@pytest.fixture(scope="module")
def sets(renderers, blob):
    feat = renderers["default"].features(_cam(), W, H)
    assert (feat["prim"] >= 0).sum() > W * H // 2
    return {"a": iref.set_floor(W, H), "b": iref.set_triangles(blob[0].arrays(), W, H), "c": iref.set_features(feat),
            "d": iref.set_mixed(feat), "e": iref.set_irregular(feat, W, H)}


def _ref(osc, sets, name, integrator, spp=SPP):
    """(f32 image, trace count) of the restatement over set `name` (computed once, shared, read-only)."""
    p, n = sets[name]
    img, cnt = iref.render_cached("cornell/" + name, osc, p, n, W, H, spp, BOUNCES, integrator, SEED)
    return np.asarray(img).astype(F), cnt["traces"]


def _dev(p, n):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([p, n], axis=1), dtype=F)).cuda()


# ---- the point sets on both integrators, and the stats
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_point_sets(renderers, osc, blob, sets, name, integrator):
    p, n = sets[name]
    r, o_sc = (blob[1], blob[2]) if name == "b" else (renderers["default"], osc)
    ref, traces = _ref(o_sc, sets, name, integrator)
    img, st = r.render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED)
    print("set %s integrator %d: differing %d, samples %d, rays_reference %d (restatement %d), rays_traced %d, work_units %d, "
          "accel_fallbacks %d" % (name, integrator, iref.same_bits(img, ref), st["samples"], st["rays_reference"], traces,
                                  st["rays_traced"], st["work_units"], st["accel_fallbacks"]))
    assert iref.same_bits(img, ref) == 0, (name, integrator)
    assert st["samples"] == W * H * SPP
    assert st["rays_reference"] == traces
    assert (st["work_units"] > 0) == (name != "e")          # a to d: the wavefront kernels; e: the whole render on the tile kernel
    if name == "d":
        assert st["accel_fallbacks"] > 0                     # the 2^-60 coordinates took the exact culled walk, lane by lane
    assert np.count_nonzero(ref) > W * H // 4                # (the set sees the light)
    if name == "e":                                          # e differs from c in the point it moved, no more
        near, _ = r.render_irradiance(*sets["c"], W, H, SPP, BOUNCES, integrator, SEED)
        diff = np.any(img.reshape(-1, 3) != near.reshape(-1, 3), axis=1)
        diff[(H // 2) * W + W // 2] = False
        assert not diff.any()


def test_a_fixed_ray_render_is_something_else(renderers, sets):
    """render_rays with the normals as directions -- what a caller had before -- is not this render."""
    p, n = sets["a"]
    r = renderers["default"]
    img, _ = r.render_irradiance(p, n, W, H, SPP, BOUNCES, 0, SEED)
    fixed, _ = r.render_rays(p, n, W, H, SPP, BOUNCES, 0, SEED)
    assert np.any(img != fixed, axis=2).sum() > W * H // 4


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_split_units_and_flags(renderers, osc, sets, name, integrator):
    p, n = sets[name]
    ref, traces = _ref(osc, sets, name, integrator)
    # PT_WF_CHUNKS=3: split units and the replayed streams (a pair and the integrator's draws per skipped sample)
    img, st = renderers["chunks"].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED)
    assert st["split_pixels"] > 0 and st["work_units"] > W * H and st["samples"] == W * H * SPP
    assert iref.same_bits(img, ref) == 0, ("chunks", name)
    ref7 = np.asarray(iref.render_cached("cornell/" + name, osc, p, n, W, H, 7, BOUNCES, integrator, SEED)[0]).astype(F)
    img, st = renderers["chunks"].render_irradiance(p, n, W, H, 7, BOUNCES, integrator, SEED)
    assert st["split_pixels"] > 0 and iref.same_bits(img, ref7) == 0, ("chunks 7 spp", name)
    # whole-pixel units
    img, base = renderers["whole"].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED)
    assert base["split_pixels"] == 0 and base["work_units"] == W * H and iref.same_bits(img, ref) == 0, ("whole", name)
    for which in ("default", "chunks", "whole"):
        plain, pst = renderers[which].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED)
        # no sample-invariant ray, no memo: PT_FLAG_NO_PRIMARY_CACHE changes neither the image nor what is traced
        img, st = renderers[which].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED, NPC)
        assert iref.same_bits(img, ref) == 0 and st["work_units"] > 0, (which, "no primary cache", name)
        assert st["rays_traced"] == pst["rays_traced"] and st["rays_reference"] == traces, (which, name)
        img, st = renderers[which].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED, NDPS)
        assert iref.same_bits(img, ref) == 0 and st["work_units"] > 0, (which, "no dead path skip", name)
        img, st = renderers[which].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED, NDPS | NPC)
        assert iref.same_bits(img, ref) == 0, (which, "both", name)
        if integrator == 0:
            assert st["rays_traced"] == traces                # every trace() of the loop, and no other


# ---- the tile paths
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "c"])
def test_tile_paths(renderers, osc, sets, name, integrator):
    p, n = sets[name]
    ref, traces = _ref(osc, sets, name, integrator)
    cases = [("default", RT), ("default", RB), ("default", RT | NPC | NDPS), ("chunks", RB)]
    if integrator == 1:
        cases += [("tile_head", 0), ("tile_head", NPC)]
    for which, flags in cases:
        img, st = renderers[which].render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED, flags)
        assert st["work_units"] == 0 and st["samples"] == W * H * SPP, (which, flags)
        assert st["rays_reference"] == traces
        assert iref.same_bits(img, ref) == 0, (name, integrator, which, flags)
    if integrator == 0:                                      # integrator 0 is not moved by PT_HEAD_WF=0
        img, st = renderers["tile_head"].render_irradiance(p, n, W, H, SPP, BOUNCES, 0, SEED)
        assert st["work_units"] > 0 and iref.same_bits(img, ref) == 0


def test_non_default_occupancy_is_refused(scene, sets):
    p, n = sets["a"]
    for env, integrator in (({"PT_WF_MIN_WAVES": "4"}, 0), ({"PT_WF_MIN_WAVES": "6"}, 0), ({"PT_HEAD_MIN_WAVES": "4"}, 1)):
        r = _renderer(scene, env)
        try:
            with pytest.raises(pt.PtError) as e:
                r.render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED)
            assert e.value.code == pt.PT_E_INVALID and "MIN_WAVES" in str(e.value)
            img, st = r.render_irradiance(p, n, W, H, 1, BOUNCES, integrator, SEED, RT)    # the tile kernel has no such knob
            assert st["work_units"] == 0 and st["samples"] == W * H
        finally:
            r.close()


# ---- geometry
@pytest.fixture(scope="module")
def frame37(renderers, osc):
    w, h = 37, 19
    p, n, _ = feature_points(renderers["default"].features(_cam(w, h), w, h), iref.LIFT)
    refs = {i: np.asarray(iref.render(osc, p, n, w, h, SPP, BOUNCES, i, SEED)).astype(F) for i in (0, 1)}
    return w, h, p, n, refs


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("count,tile", [(2, (0, 0)), (3, (16, 8)), (2, (16, 24))])
def test_shards_sum_to_the_frame(renderers, frame37, count, tile, integrator):
    w, h, p, n, refs = frame37
    ref = refs[integrator]
    r = renderers["default"]
    total = np.zeros_like(ref)
    owned = np.zeros(w * h, dtype=np.int32)
    for k in range(count):
        img, st = r.render_irradiance(p, n, w, h, SPP, BOUNCES, integrator, SEED, shard_index=k, shard_count=count,
                                      tile_w=tile[0], tile_h=tile[1])
        mine = shard.shard_pixels(w, h, k, count, tile[0], tile[1])
        owned[mine] += 1
        assert 0 < len(mine) < w * h and st["samples"] == len(mine) * SPP
        want = np.zeros_like(ref)
        want.reshape(-1, 3)[mine] = ref.reshape(-1, 3)[mine]
        assert iref.same_bits(img, want) == 0, (k, count, tile)       # the host call writes the other pixels as 0
        total += img
    assert (owned == 1).all() and iref.same_bits(total, ref) == 0
    img, st = r.render_irradiance(p, n, w, h, SPP, BOUNCES, integrator, SEED, tile_w=16, tile_h=24)
    assert iref.same_bits(img, ref) == 0 and st["samples"] == w * h * SPP


def test_device_call_writes_only_its_shard_and_an_empty_shard_nothing(renderers, frame37):
    w, h, p, n, refs = frame37
    r = renderers["default"]
    dp = _dev(p, n)
    for integrator in (0, 1):
        out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
        st = r.render_irradiance_device(dp.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, integrator, SEED, shard_index=1,
                                        shard_count=2)
        mine = shard.shard_pixels(w, h, 1, 2)
        want = np.full((w * h, 3), SENTINEL, dtype=F)
        want[mine] = refs[integrator].reshape(-1, 3)[mine]
        assert iref.same_bits(out.cpu().numpy().reshape(-1, 3), want) == 0 and st["samples"] == len(mine) * SPP
        # an empty shard (index >= tile count): d_out untouched, zero stats -- on the wavefront and on the tile path
        for flags in (0, RT):
            out.fill_(SENTINEL)
            st = r.render_irradiance_device(dp.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, integrator, SEED, flags,
                                            shard_index=7, shard_count=8, tile_w=256, tile_h=256)
            assert (out.cpu().numpy() == F(SENTINEL)).all()
            assert st["samples"] == 0 and st["rays_traced"] == 0 and st["rays_reference"] == 0 and st["work_units"] == 0
        out.fill_(SENTINEL)                                  # spp == 0 launches nothing either
        st = r.render_irradiance_device(dp.data_ptr(), out.data_ptr(), w, h, 0, BOUNCES, integrator, SEED)
        assert (out.cpu().numpy() == F(SENTINEL)).all() and st["samples"] == 0
    # the host and the device variants agree, on a stream of the caller's too
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    r.render_irradiance_device(dp.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, 0, SEED)
    host, _ = r.render_irradiance(p, n, w, h, SPP, BOUNCES, 0, SEED)
    assert iref.same_bits(out.cpu().numpy(), host) == 0 and iref.same_bits(host, refs[0]) == 0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out.zero_()
        r.render_irradiance_device(dp.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, 1, SEED, stream_ptr=s.cuda_stream)
    torch.cuda.synchronize()
    assert iref.same_bits(out.cpu().numpy(), refs[1]) == 0


@pytest.mark.parametrize("integrator", [0, 1])
def test_morton_order(renderers, osc, integrator):
    m = 16
    p, n, _ = feature_points(renderers["default"].features(_cam(m, m), m, m), iref.LIFT)
    ref = np.asarray(iref.render(osc, p, n, m, m, 3, BOUNCES, integrator, SEED)).astype(F)
    img, st = renderers["default"].render_irradiance(iref.to_morton(p, m), iref.to_morton(n, m), m, m, 3, BOUNCES, integrator,
                                                     SEED, pixel_order=pt.PT_ORDER_MORTON)
    assert img.shape == (m * m, 3) and st["samples"] == m * m * 3
    assert iref.same_bits(img, iref.to_morton(ref.reshape(-1, 3), m)) == 0
    # (scanline points under a Morton render would be other pixels' points)
    wrong, _ = renderers["default"].render_irradiance(p, n, m, m, 3, BOUNCES, integrator, SEED, pixel_order=pt.PT_ORDER_MORTON)
    assert iref.same_bits(wrong, img) > 0


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("size", [(100, 1), (1, 1)])
def test_thin_images(renderers, osc, size, integrator):
    w, h = size
    p, n = grid_points((-0.9, 0.0, 0.3), (0.0, 0.0, 0.1), (1.8, 0.0, 0.0), w, h, iref.LIFT)
    ref, cnt = iref.render(osc, p, n, w, h, SPP, BOUNCES, integrator, SEED, return_counters=True)
    for which, flags in (("default", 0), ("chunks", 0), ("default", RT)):
        img, st = renderers[which].render_irradiance(p, n, w, h, SPP, BOUNCES, integrator, SEED, flags)
        assert img.shape == (h, w, 3) and st["samples"] == w * h * SPP and st["rays_reference"] == cnt["traces"]
        assert iref.same_bits(img, ref.astype(F)) == 0, (size, which, flags)
    if size == (100, 1):
        assert np.count_nonzero(ref) > 0


# ---- a scene with spheres and nine lights (more than the kLdsLights = 5 staged in LDS), two of them spheres
def test_spheres_and_nine_lights(tmp_path):
    s = pt.Scene()
    s.load_obj(ls.write_lit_soup(str(tmp_path), 100, 7), mtl_basepath=str(tmp_path) + "/")
    ls.add_random_spheres(s, 100, 6, 2)
    s.build_bvh()
    a = s.arrays()
    assert len(a["lights"]) == 9 and len(a["spheres"]) == 6
    o_sc = oracle.OracleScene(a)
    rs = np.random.RandomState(5)
    p = rs.uniform(-1.5, 1.5, (W * H, 3)).astype(F)
    n = rays._normalised(rs.normal(size=(W * H, 3)))
    n[:6] = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=F)
    with pt.Renderer(s, 0) as r:
        for integrator in (0, 1):
            ref, cnt = iref.render(o_sc, p, n, W, H, SPP, BOUNCES, integrator, SEED, return_counters=True)
            for flags in (0, RT):
                img, st = r.render_irradiance(p, n, W, H, SPP, BOUNCES, integrator, SEED, flags)
                assert iref.same_bits(img, ref.astype(F)) == 0, (integrator, flags)
                assert st["samples"] == W * H * SPP and st["rays_reference"] == cnt["traces"]
                assert (st["work_units"] > 0) == (flags == 0)
            assert np.count_nonzero(ref) > 0


# ---- refusals: PT_E_INVALID, the output buffer unchanged
def _refused(r, dp_ptr, flags=0, w=W, h=H, spp=SPP):
    out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(pt.PtError) as e:
        r.render_irradiance_device(dp_ptr, out.data_ptr(), w, h, spp, BOUNCES, 0, SEED, flags)
    assert e.value.code == pt.PT_E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == F(SENTINEL)).all()
    return str(e.value)


def test_refusals(renderers, sets):
    r = renderers["default"]
    p, n = sets["a"]
    good = _dev(p, n)
    # invalid points: a zero, a NaN and a 1.01-long normal (and a non-finite position) -- the lowest such pixel is named
    for kind, at in (("zero", 9 * W + 1), ("nan", 5 * W + 7), ("long", 2 * W + 23), ("inf_p", 11 * W + 3)):
        p2, n2 = p.copy(), n.copy()
        if kind == "zero":
            n2[at] = 0
            n2[at + 40] = 0                                   # (a later one too: the lowest is named)
        elif kind == "nan":
            n2[at, 2] = np.nan
        elif kind == "long":
            n2[at] = n[at] * F(1.01)
        else:
            p2[at, 0] = -np.inf
        bad = _dev(p2, n2)
        for spp in (SPP, 0):                                  # (invalid points are refused before "nothing to do")
            msg = _refused(r, bad.data_ptr(), spp=spp)
            assert "pixel (%d, %d)" % (at % W, at // W) in msg, msg
        host = np.full((H, W, 3), SENTINEL, dtype=F)
        with pytest.raises(pt.PtError) as e:
            r.render_irradiance(p2, n2, W, H, SPP, BOUNCES, 1, SEED, RT, out=host)
        assert e.value.code == pt.PT_E_INVALID and "pixel (%d, %d)" % (at % W, at // W) in str(e.value)
        assert (host == F(SENTINEL)).all()
    # an invalid point outside this shard's pixels still refuses the render: all W*H points are classified
    n2 = n.copy()
    n2[0] = 0
    out = torch.full((H, W, 3), SENTINEL, dtype=torch.float32, device="cuda")
    bad = _dev(p, n2)
    with pytest.raises(pt.PtError):
        r.render_irradiance_device(bad.data_ptr(), out.data_ptr(), W, H, SPP, BOUNCES, 0, SEED, shard_index=1, shard_count=2)
    # the jitter and count flags, unknown bits
    for flags in (pt.PT_FLAG_COUNT, pt.PT_FLAG_COUNT | pt.PT_FLAG_TRI_COUNTS, pt.PT_FLAG_TRI_COUNTS, pt.PT_FLAG_JITTER,
                  pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT, pt.PT_FLAG_JITTER_TENT, 0x100, 0x80000000, RT | pt.PT_FLAG_COUNT):
        assert "flags" in _refused(r, good.data_ptr(), flags), hex(flags)
    # null buffers
    assert "null" in _refused(r, 0)
    with pytest.raises(pt.PtError) as e:
        r.render_irradiance_device(good.data_ptr(), 0, W, H, SPP)
    assert e.value.code == pt.PT_E_INVALID and "null" in str(e.value)
    # a render in flight
    buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    r.render_device_async(_cam(), buf.data_ptr(), W, H, SPP, BOUNCES, 0, SEED)
    try:
        assert "in flight" in _refused(r, good.data_ptr())
        with pytest.raises(pt.PtError) as e:
            r.render_irradiance(p, n, W, H, SPP)
        assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
        with pytest.raises(pt.PtError) as e:
            r.classify_points_device(good.data_ptr(), W * H)
        assert e.value.code == pt.PT_E_INVALID
    finally:
        r.wait()
    img, _ = r.render_irradiance(p, n, W, H, SPP, BOUNCES, 0, SEED)      # and the context still renders
    assert np.count_nonzero(img) > 0


# ---- classify_points_device against the numpy restatement
def _mixed_points(m, ext, seed):
    """m valid points: positions in and far outside the scene, unit normals, some at the ends of the length band."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(-1.0, 1.0, (m, 3)).astype(F)
    n = rays._normalised(rs.normal(size=(m, 3)))
    k = np.arange(m)
    p[k % 7 == 3] *= F(100.0 * ext)                          # beyond and within 64 extents, by component
    p[k % 11 == 5, 1] = F(64.0 * ext)                         # exactly on the bound: regular
    p[k % 13 == 6, 2] = np.nextafter(F(64.0 * ext), F(1e9))   # the next float: irregular
    n[k % 19 == 4] = np.array((1, 2.0 ** -5, 0), dtype=F)     # n.n = 1 + 2^-10, the upper bound itself
    n[k % 23 == 7] = np.array((0, 1, 2.0 ** -6), dtype=F)     # n.n = 1 + 2^-12
    return p, n


def test_classify_points_device(renderers, scene):
    r = renderers["default"]
    ext = iref.scene_extent(scene.arrays())
    p, n = _mixed_points(5000, ext, 11)
    want_all, cls = iref.classify(p, n, ext)
    assert want_all["invalid"] == 0 and want_all["regular"] > 1000 and want_all["irregular"] > 500
    dp = _dev(p, n)
    for m in (0, 1, 63, 64, 65, 5000):
        want, _ = iref.classify(p[:m], n[:m], ext)
        assert r.classify_points_device(dp.data_ptr(), m) == want, m
    assert r.classify_points_device(0, 0) == dict(regular=0, irregular=0, invalid=0, first_invalid=iref.NONE)
    # invalid points of every kind, one and many, at the first, the last and the wave-boundary indices
    kinds = [lambda p2, n2, k: n2.__setitem__(k, 0), lambda p2, n2, k: n2.__setitem__((k, 1), np.inf),
             lambda p2, n2, k: n2.__setitem__(k, n2[k] * F(1.01)), lambda p2, n2, k: p2.__setitem__((k, 2), np.nan),
             lambda p2, n2, k: n2.__setitem__(k, n2[k] * F(0.99)), lambda p2, n2, k: n2.__setitem__(k, (3e38, 3e38, 0))]
    for m in (64, 65, 5000):
        places = [[0], [m - 1], [63], [min(64, m - 1)], [0, m - 1], [63, 64] if m > 64 else [62, 63],
                  list(range(m - 1, -1, -97)), list(range(m))]
        for j, at in enumerate(places):
            p2, n2 = p[:m].copy(), n[:m].copy()
            for i, k in enumerate(at):
                kinds[(i + j) % len(kinds)](p2, n2, k)
            want, _ = iref.classify(p2, n2, ext)
            assert want["invalid"] == len(at) and want["first_invalid"] == min(at)
            got = r.classify_points_device(_dev(p2, n2).data_ptr(), m)
            assert got == want, (m, at[:4])
    # the float32 n.n exactly on the bounds is valid, the floats beyond are not (the host test builds such normals)
    lo, hi = iref.LEN2_MIN, iref.LEN2_MAX
    n2 = np.tile(np.array((0, 1, 0), dtype=F), (64, 1))
    n2[10] = (1, 2.0 ** -5, 0)                                # n.n = 1 + 2^-10 exactly
    n2[20] = (1, np.nextafter(F(2.0 ** -5), F(1)) * F(1 + 2.0 ** -12), 0)
    want, cls = iref.classify(p[:64], n2, ext)
    assert cls[10] != 2 and cls[20] == 2 and lo < hi
    assert r.classify_points_device(_dev(p[:64], n2).data_ptr(), 64) == want
    # an unaligned buffer is refused, not misread
    with pytest.raises(pt.PtError) as e:
        r.classify_points_device(dp.data_ptr() + 4, 16)
    assert e.value.code == pt.PT_E_INVALID and "aligned" in str(e.value)


# ---- the stand-in scene: feature_points of its camera, 256 spread pixels against the restatement
@pytest.mark.parametrize("integrator", [0, 1])
def test_standin(standin_scene, integrator):
    w, h, spp = 256, 144, 2
    cam = pt.make_camera(*[scenes.SPONZA_STANDIN_CAMERA[k] for k in ("pos", "dist_from_film", "focal_length")], 0.0, w, h)
    o_sc = oracle.OracleScene(standin_scene.arrays())
    with pt.Renderer(standin_scene, 0) as r:
        p, n, miss = feature_points(r.features(cam, w, h), iref.LIFT)
        assert miss.sum() < w * h // 2
        img, st = r.render_irradiance(p, n, w, h, spp, BOUNCES, integrator, SEED)
        assert st["work_units"] > 0 and st["samples"] == w * h * spp
        pixels = (np.arange(256, dtype=np.int64) * (w * h // 256) + 37) % (w * h)
        ref = iref.render(o_sc, p, n, w, h, spp, BOUNCES, integrator, SEED, pixels=pixels)
        got = img.reshape(-1, 3)[pixels]
        assert iref.same_bits(got, ref.reshape(-1, 3)[pixels].astype(F)) == 0
        assert np.count_nonzero(got) > 0
        total = np.zeros_like(img)
        for k in range(2):
            part, pst = r.render_irradiance(p, n, w, h, spp, BOUNCES, integrator, SEED, shard_index=k, shard_count=2)
            assert 0 < pst["samples"] < w * h * spp
            total += part
        assert iref.same_bits(total, img) == 0


# ---- pt_cli --irradiance writes the image the library call returns
def _cli(*args):
    base = [CLI, "--obj", os.path.join(MODELS, "cornell.obj"), "--quiet"]
    return subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_irradiance(renderers, sets, tmp_path):
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    p, n = sets["c"]
    np.ascontiguousarray(np.concatenate([p, n], axis=1), dtype="<f4").tofile(t("c.pts"))
    size = ["--width", W, "--height", H, "--bounces", BOUNCES, "--seed", SEED, "--spp", SPP]
    r = _cli(*size, "--irradiance", t("c.pts"), "--pfm", t("c.pfm"), "--out", t("c.ppm"))
    assert r.returncode == 0, r.stderr
    img, _ = renderers["default"].render_irradiance(p, n, W, H, SPP, BOUNCES, 0, SEED)
    assert pt.read_pfm(t("c.pfm")).tobytes() == img.tobytes()
    r = _cli(*size, "--irradiance", t("c.pts"), "--integrator", "head", "--pfm", t("h.pfm"), "--out", t("h.ppm"))
    assert r.returncode == 0, r.stderr
    img, _ = renderers["default"].render_irradiance(p, n, W, H, SPP, BOUNCES, 1, SEED)
    assert pt.read_pfm(t("h.pfm")).tobytes() == img.tobytes()
    # usage errors: with --rays, with a camera option, with what --rays excludes, with the feature options
    for extra in (["--rays", t("c.pts")], ["--cam", "0,1,3"], ["--radius", 0.05], ["--look-at", "0,1,0"], ["--jitter", "box"],
                  ["--pass-spp", 2], ["--checkpoint", t("x.ptacc")], ["--vfov", 40], ["--denoise"], ["--aov", t("aov")]):
        r = _cli(*size, "--irradiance", t("c.pts"), "--out", t("x.ppm"), *extra)
        assert r.returncode == 2 and "--irradiance cannot be combined with" in r.stderr, (extra, r.stderr[:200])
    r = _cli("--width", W + 1, "--height", H, "--spp", 1, "--irradiance", t("c.pts"), "--out", t("x.ppm"))
    assert r.returncode == 2 and "does not hold" in r.stderr
    n2 = n.copy()
    n2[30] = 0
    np.ascontiguousarray(np.concatenate([p, n2], axis=1), dtype="<f4").tofile(t("bad.pts"))
    r = _cli(*size, "--irradiance", t("bad.pts"), "--out", t("x.ppm"))
    assert r.returncode == 1 and "pixel (6, 1)" in r.stderr
    assert not os.path.exists(t("x.ppm"))
