"""Renders along caller-supplied rays on the GPU (include/pt/pt.h, pt_render_rays*, pt_rays_classify_device): every image
equals rays_ref -- the oracle's per-pixel loop restated around the ray buffer, no lens draws -- in every bit, on the
wavefront kernels (both integrators, split units, the memo off), on the tile kernel (the reference flags, PT_HEAD_WF=0,
an irregular buffer) and through every shard / tile / order geometry; the classification kernel equals its numpy
restatement.  Cornell box, 24 x 16, 4 samples, 3 bounces, seed 1234 unless said otherwise."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import MODELS, ROOT, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import rays, scenes, shard          # (the parent has no rays module: every test here errors there)
import light_scenes as ls
import oracle
import rays_ref

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, SPP, BOUNCES, SEED = 24, 16, 4, 3, 1234
POS = rays_ref.POS
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
def sets():
    return {"a": rays_ref.set_camera(pt, W, H), "b": rays_ref.set_ortho(W, H), "c": rays_ref.set_panorama(W, H),
            "d": rays_ref.set_probes(W, H), "e": rays_ref.set_mixed(pt, W, H), "f": rays_ref.set_irregular(pt, W, H)}


def _ref(osc, sets, name, integrator, spp=SPP):
    """(f32 image, trace count) of the restatement over set `name` (computed once, shared, read-only)."""
    o, d = sets[name]
    img, cnt = rays_ref.render_cached("cornell/" + name, osc, o, d, W, H, spp, BOUNCES, integrator, SEED)
    return np.asarray(img).astype(F), cnt["traces"]


def _cam(w=W, h=H):
    return pt.make_camera(POS, 1.0, 3.0, 0.0, w, h)


def _dev(o, d):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=F)).cuda()


def _except_pixel0(img, plain):
    """Differing values outside pixel (0, 0) of two (H, W, 3) images."""
    diff = img.view(np.uint32) != plain.view(np.uint32)
    diff[0, 0] = False
    return int(np.count_nonzero(diff))


# ---- 5. the ray sets on both integrators, 9. the stats
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_ray_sets(renderers, osc, sets, name, integrator):
    o, d = sets[name]
    r = renderers["default"]
    ref, traces = _ref(osc, sets, name, integrator)
    img, st = r.render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED)
    print("set %s integrator %d: differing %d, samples %d, rays_reference %d (restatement %d), rays_traced %d, work_units %d, "
          "accel_fallbacks %d" % (name, integrator, rays_ref.same_bits(img, ref), st["samples"], st["rays_reference"], traces,
                                  st["rays_traced"], st["work_units"], st["accel_fallbacks"]))
    assert rays_ref.same_bits(img, ref) == 0, (name, integrator)
    assert st["samples"] == W * H * SPP
    assert st["rays_reference"] == traces
    assert (st["work_units"] > 0) == (name != "f")          # a to e: the wavefront kernels; f: the whole render on the tile kernel
    if name == "e":
        assert st["accel_fallbacks"] > 0                     # the 2^-60 origins took the exact culled walk, lane by lane
    assert np.count_nonzero(ref) > W * H // 4                # (the set sees the scene)
    if name in ("a", "f"):
        plain, pst = r.render(_cam(), W, H, SPP, BOUNCES, integrator, SEED)
        if name == "a":
            assert _except_pixel0(img, plain) == 0
        else:                                                # f differs from a in the two rays it moved, no more
            k = (H // 2) * W + W // 2
            diff = np.any(img.reshape(-1, 3) != plain.reshape(-1, 3), axis=1)
            diff[[0, k, k + 1]] = False
            assert not diff.any()


def test_rays_traced_with_the_memo_on(renderers, osc):
    """rays_traced of the camera's own rays is the plain render's minus the difference at pixel (0, 0).  Every other
    pixel does what it does in the plain render.  With this wider camera pixel (0, 0)'s ray misses the scene (asserted
    with the oracle), so each of its samples is one primary trace and a dead path, whatever its stream: the plain
    render, where it is a lens pixel without memo, traces the ray SPP times; this one traces it once.
    On a renderer of whole-pixel units (PT_WF_CHUNKS=1), where the memo is the unit's own: between the chunks of a split
    pixel it is shared only when the owner happens to have published it in time, so the default renderer's count at
    this size depends on the timing (measured: plain 1499, rays 1725, no memo 1725)."""
    cam = pt.make_camera(POS, 0.5, 3.0, 0.0, W, H)
    o, d = rays.camera_rays(cam)
    tri, _ = oracle.trace_batch(osc, o[:1], d[:1])
    assert tri[0] == -1
    r = renderers["whole"]
    plain, pst = r.render(cam, W, H, SPP, BOUNCES, 0, SEED)
    img, st = r.render_rays(o, d, W, H, SPP, BOUNCES, 0, SEED)
    assert st["split_pixels"] == 0 and st["work_units"] == W * H
    print("rays_traced: plain %d, rays %d" % (pst["rays_traced"], st["rays_traced"]))
    assert rays_ref.same_bits(img, plain) == 0 and np.count_nonzero(img) > W * H // 4
    assert pst["rays_traced"] - st["rays_traced"] == SPP - 1
    assert pst["rays_reference"] == st["rays_reference"]
    # and with the memo off both trace the same rays
    pst = r.render(cam, W, H, SPP, BOUNCES, 0, SEED, NPC)[1]
    st = r.render_rays(o, d, W, H, SPP, BOUNCES, 0, SEED, NPC)[1]
    assert pst["rays_traced"] == st["rays_traced"]
    # set a itself (the other suites' camera; its pixel (0, 0) hits a wall, so what that pixel traces depends on its
    # stream): every 8 x 8 tile but the one that holds pixel (0, 0) traces what it traces in the plain render
    cam = _cam()
    o, d = rays.camera_rays(cam)
    for integrator in (0, 1):
        for k in range(6):
            pst = r.render(cam, W, H, SPP, BOUNCES, integrator, SEED, shard_index=k, shard_count=6)[1]
            st = r.render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, shard_index=k, shard_count=6)[1]
            assert pst["samples"] == st["samples"] == 64 * SPP and st["split_pixels"] == 0
            if k > 0:
                assert pst["rays_traced"] == st["rays_traced"], (integrator, k)
            assert pst["rays_reference"] == st["rays_reference"] or k == 0


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "e", "c"])
def test_split_units_and_flags(renderers, osc, sets, name, integrator):
    o, d = sets[name]
    ref, traces = _ref(osc, sets, name, integrator)
    # PT_WF_CHUNKS=3: split units, the replayed streams and the pixels' shared memo
    img, st = renderers["chunks"].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED)
    assert st["split_pixels"] > 0 and st["work_units"] > W * H and st["samples"] == W * H * SPP
    assert rays_ref.same_bits(img, ref) == 0, ("chunks", name)
    ref7 = np.asarray(rays_ref.render_cached("cornell/" + name, osc, o, d, W, H, 7, BOUNCES, integrator, SEED)[0]).astype(F)
    img, st = renderers["chunks"].render_rays(o, d, W, H, 7, BOUNCES, integrator, SEED)
    assert st["split_pixels"] > 0 and rays_ref.same_bits(img, ref7) == 0, ("chunks 7 spp", name)
    # whole-pixel units: the unit's own memo (deterministic: every pixel traces its ray once instead of SPP times)
    img, base = renderers["whole"].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED)
    assert base["split_pixels"] == 0 and rays_ref.same_bits(img, ref) == 0, ("whole", name)
    img, st = renderers["whole"].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, NPC)
    assert rays_ref.same_bits(img, ref) == 0 and st["rays_traced"] == base["rays_traced"] + W * H * (SPP - 1), ("whole", name)
    for which in ("default", "chunks"):
        img, st = renderers[which].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, NPC)
        assert rays_ref.same_bits(img, ref) == 0 and st["work_units"] > 0, (which, "no primary cache", name)
        assert st["rays_reference"] == traces
        img, st = renderers[which].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, NDPS)
        assert rays_ref.same_bits(img, ref) == 0 and st["work_units"] > 0, (which, "no dead path skip", name)
        img, st = renderers[which].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, NDPS | NPC)
        assert rays_ref.same_bits(img, ref) == 0, (which, "both", name)
        if integrator == 0:
            assert st["rays_traced"] == traces                # every trace() of the loop, and no other


# ---- 6. the tile paths
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "c"])
def test_tile_paths(renderers, osc, sets, name, integrator):
    o, d = sets[name]
    ref, traces = _ref(osc, sets, name, integrator)
    cases = [("default", RT), ("default", RB), ("default", RT | NPC | NDPS), ("chunks", RB)]
    if integrator == 1:
        cases += [("tile_head", 0), ("tile_head", NPC)]
    for which, flags in cases:
        img, st = renderers[which].render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, flags)
        assert st["work_units"] == 0 and st["samples"] == W * H * SPP, (which, flags)
        assert st["rays_reference"] == traces
        assert rays_ref.same_bits(img, ref) == 0, (name, integrator, which, flags)
    # integrator 0 is not moved by PT_HEAD_WF=0
    if integrator == 0:
        img, st = renderers["tile_head"].render_rays(o, d, W, H, SPP, BOUNCES, 0, SEED)
        assert st["work_units"] > 0 and rays_ref.same_bits(img, ref) == 0


def test_non_default_occupancy_is_refused(scene, sets):
    o, d = sets["a"]
    for env, integrator in (({"PT_WF_MIN_WAVES": "4"}, 0), ({"PT_WF_MIN_WAVES": "6"}, 0), ({"PT_HEAD_MIN_WAVES": "4"}, 1)):
        r = _renderer(scene, env)
        try:
            with pytest.raises(pt.PtError) as e:
                r.render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED)
            assert e.value.code == pt.PT_E_INVALID and "MIN_WAVES" in str(e.value)
            img, st = r.render_rays(o, d, W, H, 1, BOUNCES, integrator, SEED, RT)     # the tile kernel has no such knob
            assert st["work_units"] == 0 and st["samples"] == W * H
        finally:
            r.close()


# ---- 7. geometry
@pytest.fixture(scope="module")
def frame37(osc):
    w, h = 37, 19
    o, d = rays.camera_rays(_cam(w, h))
    refs = {i: np.asarray(rays_ref.render(osc, o, d, w, h, SPP, BOUNCES, i, SEED)).astype(F) for i in (0, 1)}
    return w, h, o, d, refs


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("count,tile", [(2, (0, 0)), (3, (16, 8)), (2, (16, 24))])
def test_shards_sum_to_the_frame(renderers, frame37, count, tile, integrator):
    w, h, o, d, refs = frame37
    ref = refs[integrator]
    r = renderers["default"]
    total = np.zeros_like(ref)
    owned = np.zeros(w * h, dtype=np.int32)
    for k in range(count):
        img, st = r.render_rays(o, d, w, h, SPP, BOUNCES, integrator, SEED, shard_index=k, shard_count=count, tile_w=tile[0],
                                tile_h=tile[1])
        mine = shard.shard_pixels(w, h, k, count, tile[0], tile[1])
        owned[mine] += 1
        assert 0 < len(mine) < w * h and st["samples"] == len(mine) * SPP
        want = np.zeros_like(ref)
        want.reshape(-1, 3)[mine] = ref.reshape(-1, 3)[mine]
        assert rays_ref.same_bits(img, want) == 0, (k, count, tile)     # the host call writes the other pixels as 0
        total += img
    assert (owned == 1).all() and rays_ref.same_bits(total, ref) == 0
    # a 16 x 24 tile on the whole 37 x 19 image (partial tiles right and below)
    img, st = r.render_rays(o, d, w, h, SPP, BOUNCES, integrator, SEED, tile_w=16, tile_h=24)
    assert rays_ref.same_bits(img, ref) == 0 and st["samples"] == w * h * SPP


def test_device_call_writes_only_its_shard_and_an_empty_shard_nothing(renderers, frame37):
    w, h, o, d, refs = frame37
    r = renderers["default"]
    dr = _dev(o, d)
    for integrator in (0, 1):
        out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
        st = r.render_rays_device(dr.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, integrator, SEED, shard_index=1, shard_count=2)
        mine = shard.shard_pixels(w, h, 1, 2)
        want = np.full((w * h, 3), SENTINEL, dtype=F)
        want[mine] = refs[integrator].reshape(-1, 3)[mine]
        assert rays_ref.same_bits(out.cpu().numpy().reshape(-1, 3), want) == 0 and st["samples"] == len(mine) * SPP
        # an empty shard (index >= tile count): d_out untouched, zero stats -- on the wavefront and on the tile path
        for flags in (0, RT):
            out.fill_(SENTINEL)
            st = r.render_rays_device(dr.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, integrator, SEED, flags, shard_index=7,
                                      shard_count=8, tile_w=256, tile_h=256)
            assert (out.cpu().numpy() == F(SENTINEL)).all()
            assert st["samples"] == 0 and st["rays_traced"] == 0 and st["rays_reference"] == 0 and st["work_units"] == 0
        # spp == 0 launches nothing either
        out.fill_(SENTINEL)
        st = r.render_rays_device(dr.data_ptr(), out.data_ptr(), w, h, 0, BOUNCES, integrator, SEED)
        assert (out.cpu().numpy() == F(SENTINEL)).all() and st["samples"] == 0
    # the host and the device variants agree (13)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    r.render_rays_device(dr.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, 0, SEED)
    host, _ = r.render_rays(o, d, w, h, SPP, BOUNCES, 0, SEED)
    assert rays_ref.same_bits(out.cpu().numpy(), host) == 0 and rays_ref.same_bits(host, refs[0]) == 0
    # ... on a stream of the caller's too
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out.zero_()
        r.render_rays_device(dr.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, 1, SEED, stream_ptr=s.cuda_stream)
    torch.cuda.synchronize()
    assert rays_ref.same_bits(out.cpu().numpy(), refs[1]) == 0


@pytest.mark.parametrize("integrator", [0, 1])
def test_morton_order(renderers, osc, integrator):
    n = 16
    o, d = rays.camera_rays(_cam(n, n))
    ref = np.asarray(rays_ref.render(osc, o, d, n, n, 3, BOUNCES, integrator, SEED)).astype(F)
    # the ray buffer in Morton order, like the image
    img, st = renderers["default"].render_rays(rays_ref.to_morton(o, n), rays_ref.to_morton(d, n), n, n, 3, BOUNCES, integrator, SEED,
                                               pixel_order=pt.PT_ORDER_MORTON)
    assert img.shape == (n * n, 3) and st["samples"] == n * n * 3
    assert rays_ref.same_bits(img, rays_ref.to_morton(ref.reshape(-1, 3), n)) == 0
    # (scanline rays under a Morton render would be other pixels' rays)
    wrong, _ = renderers["default"].render_rays(o, d, n, n, 3, BOUNCES, integrator, SEED, pixel_order=pt.PT_ORDER_MORTON)
    assert rays_ref.same_bits(wrong, img) > 0
    with pytest.raises(pt.PtError):
        renderers["default"].render_rays(o[:15 * 16], d[:15 * 16], 16, 15, 1, pixel_order=pt.PT_ORDER_MORTON)


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("size", [(100, 1), (1, 1), (1, 9)])
def test_thin_images(renderers, osc, size, integrator):
    w, h = size
    o, d = rays.panorama_rays((0.1, 0.9, 0.2), w, h)
    if (w, h) == (1, 1):
        o, d = np.array([[0.0, 1.0, 3.0]], dtype=F), np.array([[0.0, 0.0, -1.0]], dtype=F)
    ref, cnt = rays_ref.render(osc, o, d, w, h, SPP, BOUNCES, integrator, SEED, return_counters=True)
    for which, flags in (("default", 0), ("chunks", 0), ("default", RT)):
        img, st = renderers[which].render_rays(o, d, w, h, SPP, BOUNCES, integrator, SEED, flags)
        assert img.shape == (h, w, 3) and st["samples"] == w * h * SPP and st["rays_reference"] == cnt["traces"]
        assert rays_ref.same_bits(img, ref.astype(F)) == 0, (size, which, flags)
    assert np.count_nonzero(ref) > 0


# ---- 8. scenes
def _scene_case(name, tmp):
    if name == "cornell_spheres":
        s = load_scene("cornell", build_bvh=False)
        scenes.add_cornell_spheres(s)
    else:                               # nine emissive triangles: more than the kLdsLights = 5 staged in LDS
        s = pt.Scene()
        s.load_obj(ls.write_lit_soup(tmp, 100, 9), mtl_basepath=tmp + "/")
    s.build_bvh()
    return s


@pytest.mark.parametrize("name", ["cornell_spheres", "lit_soup_9_lights"])
def test_scene_kinds(tmp_path, name):
    s = _scene_case(name, str(tmp_path))
    a = s.arrays()
    if name == "lit_soup_9_lights":
        assert len(a["lights"]) == 9
    else:
        assert len(a["spheres"]) > 0
    o_sc = oracle.OracleScene(a)
    sets_ = {"camera": rays_ref.set_camera(pt, W, H), "panorama": rays_ref.set_panorama(W, H)}
    with pt.Renderer(s, 0) as r:
        for sname, (o, d) in sets_.items():
            for integrator in (0, 1):
                ref, cnt = rays_ref.render(o_sc, o, d, W, H, SPP, BOUNCES, integrator, SEED, return_counters=True)
                for flags in (0, RT):
                    img, st = r.render_rays(o, d, W, H, SPP, BOUNCES, integrator, SEED, flags)
                    assert rays_ref.same_bits(img, ref.astype(F)) == 0, (name, sname, integrator, flags)
                    assert st["samples"] == W * H * SPP and st["rays_reference"] == cnt["traces"]
                    assert (st["work_units"] > 0) == (flags == 0)
                assert np.count_nonzero(ref) > 0


# ---- 10. refusals: PT_E_INVALID, the output buffer unchanged
def _refused(r, dr_ptr, flags=0, w=W, h=H, spp=SPP):
    out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(pt.PtError) as e:
        r.render_rays_device(dr_ptr, out.data_ptr(), w, h, spp, BOUNCES, 0, SEED, flags)
    assert e.value.code == pt.PT_E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == F(SENTINEL)).all()
    return str(e.value)


def test_refusals(renderers, sets):
    r = renderers["default"]
    o, d = sets["a"]
    good = _dev(o, d)
    # invalid rays: a NaN, an infinity, a zero direction -- the message names the lowest such pixel
    for kind, at in (("nan", 5 * W + 7), ("inf", 2 * W + 23), ("zero", 9 * W + 1)):
        o2, d2 = o.copy(), d.copy()
        if kind == "nan":
            o2[at, 2] = np.nan
        elif kind == "inf":
            d2[at, 0] = -np.inf
        else:
            d2[at] = 0
            d2[at + 40] = 0                                   # (a later one too: the lowest is named)
        bad = _dev(o2, d2)
        for spp in (SPP, 0):                                  # (invalid rays are refused before "nothing to do")
            msg = _refused(r, bad.data_ptr(), spp=spp)
            assert "pixel (%d, %d)" % (at % W, at // W) in msg, msg
        host = np.full((H, W, 3), SENTINEL, dtype=F)
        with pytest.raises(pt.PtError) as e:
            r.render_rays(o2, d2, W, H, SPP, BOUNCES, 1, SEED, RT, out=host)
        assert e.value.code == pt.PT_E_INVALID and "pixel (%d, %d)" % (at % W, at // W) in str(e.value)
        assert (host == F(SENTINEL)).all()
    # an invalid ray outside this shard's pixels still refuses the render: all W*H rays are classified
    o2 = o.copy()
    o2[0, 0] = np.inf
    out = torch.full((H, W, 3), SENTINEL, dtype=torch.float32, device="cuda")
    bad = _dev(o2, d)
    with pytest.raises(pt.PtError):
        r.render_rays_device(bad.data_ptr(), out.data_ptr(), W, H, SPP, BOUNCES, 0, SEED, shard_index=1, shard_count=2)
    # in a Morton-ordered buffer the index is a Morton index
    n = 16
    mo, md = rays.camera_rays(_cam(n, n))
    mo, md = rays_ref.to_morton(mo, n), rays_ref.to_morton(md, n)
    md[rays_ref.morton(5, 9)] = 0
    out16 = torch.full((n * n, 3), SENTINEL, dtype=torch.float32, device="cuda")
    bad = _dev(mo, md)
    with pytest.raises(pt.PtError) as e:
        r.render_rays_device(bad.data_ptr(), out16.data_ptr(), n, n, SPP, pixel_order=pt.PT_ORDER_MORTON)
    assert "pixel (5, 9)" in str(e.value) and (out16.cpu().numpy() == F(SENTINEL)).all()
    # the refused flags, and an unknown bit
    for flags in (pt.PT_FLAG_COUNT, pt.PT_FLAG_COUNT | pt.PT_FLAG_TRI_COUNTS, pt.PT_FLAG_TRI_COUNTS, pt.PT_FLAG_JITTER,
                  pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT, pt.PT_FLAG_JITTER_TENT, 0x100, 0x80000000, RT | pt.PT_FLAG_COUNT):
        assert "flags" in _refused(r, good.data_ptr(), flags), hex(flags)
    # null buffers
    assert "null" in _refused(r, 0)
    with pytest.raises(pt.PtError) as e:
        r.render_rays_device(good.data_ptr(), 0, W, H, SPP)
    assert e.value.code == pt.PT_E_INVALID and "null" in str(e.value)
    # a render in flight
    buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    r.render_device_async(_cam(), buf.data_ptr(), W, H, SPP, BOUNCES, 0, SEED)
    try:
        assert "in flight" in _refused(r, good.data_ptr())
        with pytest.raises(pt.PtError) as e:
            r.render_rays(o, d, W, H, SPP)
        assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
        with pytest.raises(pt.PtError) as e:
            r.classify_rays_device(good.data_ptr(), W * H)
        assert e.value.code == pt.PT_E_INVALID
    finally:
        r.wait()
    # and the context still renders
    img, _ = r.render_rays(o, d, W, H, SPP, BOUNCES, 0, SEED)
    assert np.count_nonzero(img) > 0


# ---- 11. classify_rays_device against the numpy restatement
def _mixed_rays(n, ext, seed):
    """n rays of all valid kinds: origins in and far outside the scene, directions normalised, short and long."""
    rs = np.random.RandomState(seed)
    o = rs.uniform(-1.0, 1.0, (n, 3)).astype(F)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    k = np.arange(n)
    o[k % 7 == 3] *= F(100.0 * ext)                          # beyond and within 64 extents, by component
    o[k % 11 == 5, 1] = F(64.0 * ext)                         # exactly on the bound: regular
    o[k % 13 == 6, 2] = np.nextafter(F(64.0 * ext), F(1e9))   # the next float: irregular
    d[k % 5 == 1] *= F(2.0)
    d[k % 17 == 2] *= F(0.25)
    d[k % 19 == 4] = np.array((np.sqrt(rays_ref.DIR_LEN2_MAX), 0, 0), dtype=F)
    d[k % 23 == 7] = np.array((3e38, -3e38, 0), dtype=F)      # |d|^2 overflows: irregular, not invalid
    return o, d


def test_classify_rays_device(renderers, scene):
    r = renderers["default"]
    ext = rays_ref.scene_extent(scene.arrays())
    o, d = _mixed_rays(5000, ext, 11)
    want_all, cls = rays_ref.classify(o, d, ext)
    assert want_all["invalid"] == 0 and want_all["regular"] > 1000 and want_all["irregular"] > 1000
    dr = _dev(o, d)
    for n in (0, 1, 63, 64, 65, 256, 257, 5000):
        want, _ = rays_ref.classify(o[:n], d[:n], ext)
        assert r.classify_rays_device(dr.data_ptr(), n) == want, n
    assert r.classify_rays_device(0, 0) == dict(regular=0, irregular=0, invalid=0, first_invalid=rays_ref.NONE)
    # invalid rays: one and many, at the first, the last and the wave-boundary indices
    kinds = [lambda o2, d2, k: o2.__setitem__((k, 0), np.nan), lambda o2, d2, k: d2.__setitem__((k, 1), np.inf),
             lambda o2, d2, k: d2.__setitem__(k, 0), lambda o2, d2, k: o2.__setitem__((k, 2), -np.inf)]
    for n in (64, 65, 257, 5000):
        places = [[0], [n - 1], [63], [min(64, n - 1)], [0, n - 1], [63, 64] if n > 64 else [62, 63],
                  list(range(n - 1, -1, -97)), list(range(n))]
        for j, at in enumerate(places):
            o2, d2 = o[:n].copy(), d[:n].copy()
            for i, k in enumerate(at):
                kinds[(i + j) % 4](o2, d2, k)
            want, _ = rays_ref.classify(o2, d2, ext)
            assert want["invalid"] == len(at) and want["first_invalid"] == min(at)
            dr2 = _dev(o2, d2)
            got = r.classify_rays_device(dr2.data_ptr(), n)
            assert got == want, (n, at[:4])
    # a direction of (0, -0, 0) is a zero direction; a denormal one is not
    o2, d2 = o[:64].copy(), d[:64].copy()
    d2[10] = np.array((0.0, -0.0, 0.0), dtype=F)
    d2[20] = np.array((0.0, 1e-45, 0.0), dtype=F)
    want, _ = rays_ref.classify(o2, d2, ext)
    assert want["invalid"] == 1 and want["first_invalid"] == 10
    dr2 = _dev(o2, d2)
    assert r.classify_rays_device(dr2.data_ptr(), 64) == want
    # an unaligned buffer is refused, not misread
    with pytest.raises(pt.PtError) as e:
        r.classify_rays_device(dr.data_ptr() + 4, 16)
    assert e.value.code == pt.PT_E_INVALID and "aligned" in str(e.value)


# ---- 12. the stand-in scene: the check DESIGN.md 10 item 6 asks of any new integrator-1 kernel instance
@pytest.mark.parametrize("integrator", [0, 1])
def test_standin_equals_the_plain_render(standin_scene, integrator):
    w, h = 256, 144
    cam = _cam(w, h)
    o, d = rays.camera_rays(cam)
    with pt.Renderer(standin_scene, 0) as r:
        plain, pst = r.render(cam, w, h, SPP, BOUNCES, integrator, SEED)
        img, st = r.render_rays(o, d, w, h, SPP, BOUNCES, integrator, SEED)
        assert st["work_units"] > 0 and st["samples"] == w * h * SPP
        assert _except_pixel0(img, plain) == 0
        assert np.count_nonzero(plain) > w * h
        total = np.zeros_like(img)
        for k in range(2):
            part, pst2 = r.render_rays(o, d, w, h, SPP, BOUNCES, integrator, SEED, shard_index=k, shard_count=2)
            assert 0 < pst2["samples"] < w * h * SPP
            total += part
        assert rays_ref.same_bits(total, img) == 0


# ---- 13. pt_cli --rays writes the image the library call returns
def _cli(*args):
    base = [CLI, "--obj", os.path.join(MODELS, "cornell.obj"), "--quiet"]
    return subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_rays(renderers, sets, tmp_path):
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    o, d = sets["c"]
    np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype="<f4").tofile(t("c.rays"))
    size = ["--width", W, "--height", H, "--bounces", BOUNCES, "--seed", SEED, "--spp", SPP]
    r = _cli(*size, "--rays", t("c.rays"), "--pfm", t("c.pfm"), "--out", t("c.ppm"))
    assert r.returncode == 0, r.stderr
    img, _ = renderers["default"].render_rays(o, d, W, H, SPP, BOUNCES, 0, SEED)
    assert pt.read_pfm(t("c.pfm")).tobytes() == img.tobytes()
    pt.write_ppm(t("lib.ppm"), img)
    assert open(t("c.ppm"), "rb").read() == open(t("lib.ppm"), "rb").read()
    r = _cli(*size, "--rays", t("c.rays"), "--integrator", "head", "--pfm", t("h.pfm"), "--out", t("h.ppm"))
    assert r.returncode == 0, r.stderr
    img, _ = renderers["default"].render_rays(o, d, W, H, SPP, BOUNCES, 1, SEED)
    assert pt.read_pfm(t("h.pfm")).tobytes() == img.tobytes()
    # what it cannot be combined with, a file of the wrong size, an invalid ray
    for extra in (["--cam", "0,1,3"], ["--radius", 0.05], ["--look-at", "0,1,0"], ["--jitter", "box"], ["--checkpoint", t("x.ptacc")],
                  ["--session", t("x.ptses")], ["--pass-spp", 2], ["--until-error", 0.1], ["--adaptive"],
                  ["--camera-path", t("p.txt"), "--temporal"], ["--vfov", 40]):
        r = _cli(*size, "--rays", t("c.rays"), "--out", t("x.ppm"), *extra)
        assert r.returncode == 2 and "--rays cannot be combined with" in r.stderr, (extra, r.stderr[:200])
    r = _cli("--width", W + 1, "--height", H, "--spp", 1, "--rays", t("c.rays"), "--out", t("x.ppm"))
    assert r.returncode == 2 and "does not hold" in r.stderr
    d2 = d.copy()
    d2[30] = 0
    np.ascontiguousarray(np.concatenate([o, d2], axis=1), dtype="<f4").tofile(t("bad.rays"))
    r = _cli(*size, "--rays", t("bad.rays"), "--out", t("x.ppm"))
    assert r.returncode == 1 and "pixel (6, 1)" in r.stderr
    assert not os.path.exists(t("x.ppm"))
