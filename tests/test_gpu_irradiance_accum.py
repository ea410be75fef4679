"""Accumulators over caller-supplied points on the GPU (include/pt/pt.h, pt_accum_create_points*): passes in any split
equal pt_render_irradiance of the same total and irradiance_ref -- the definition's per-pixel loop, a cosine-weighted
direction per sample -- in every bit, on every unit plan and through every shard / tile / order geometry; frozen and
masked texels, the noise estimator and the two loops equal their restatements fed with irradiance_ref's means; what a
point accumulator refuses.  Cornell box, 24 x 16, 3 bounces, seed 1234 unless said otherwise.  Nothing here has a
tolerance."""
import os

import numpy as np
import pytest
import torch

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import rays, shard
from cudapathtracer_amd.rays import chart_points                                 # (the parent has none: every test here errors there)

import adaptive_ref
import denoise_guided_ref
import irradiance_accum_ref as iar
import irradiance_ref as iref
import light_scenes as ls
import noise_ref
import oracle

pytestmark = pytest.mark.gpu

F = np.float32
W, H, BOUNCES, SEED = iar.W, iar.H, iar.BOUNCES, iar.SEED
POS = iref.POS
NPC, NDPS = pt.PT_FLAG_NO_PRIMARY_CACHE, pt.PT_FLAG_NO_DEAD_PATH_SKIP
SPLIT = (1, 1, 2)                      # the passes of the equivalence cases: 4 samples in all
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


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def osc(scene):
    return oracle.OracleScene(scene.arrays())


@pytest.fixture(scope="module")
def renderers(scene):
    assert hasattr(pt.Renderer, "accumulator_points")
    rs = {"default": _renderer(scene, {}), "chunks": _renderer(scene, {"PT_WF_CHUNKS": "3"}),
          "whole": _renderer(scene, {"PT_WF_CHUNKS": "1"})}
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
def sets(renderers, blob, scene, osc):
    feat = renderers["default"].features(_cam(), W, H)
    assert (feat["prim"] >= 0).sum() > W * H // 2
    s = {"a": iref.set_floor(W, H), "b": iref.set_triangles(blob[0].arrays(), W, H), "c": iref.set_features(feat),
         "d": iref.set_mixed(feat), "e": iref.set_irregular(feat, W, H)}
    # set c is the one the host test's conditions were taken on
    host = iar.host_sets(scene.arrays(), osc)
    assert _bits(s["c"][0]) == _bits(host["c"][0]) and _bits(s["c"][1]) == _bits(host["c"][1])
    return s


def _ref(osc, sets, name, integrator, n):
    """(f64 mean, cumulative trace count) of the restatement after n samples of set `name` (computed once, read-only)."""
    p, nr = sets[name]
    img, cnt = iref.render_cached("cornell/" + name, osc, p, nr, W, H, n, BOUNCES, integrator, SEED)
    return np.asarray(img), cnt["traces"]


def _dev(p, n):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([p, n], axis=1), dtype=F)).cuda()


def _check(acc, mean):
    """The accumulator holds the f64 image `mean`: mean64() and image() in every bit."""
    assert _bits(acc.mean64()) == _bits(mean)
    assert _bits(acc.image()) == _bits(mean.astype(F))


# ---- 1. pass equivalence
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_passes_equal_the_one_shot_render(renderers, osc, blob, sets, name, integrator):
    p, n = sets[name]
    r, o_sc = (blob[1], blob[2]) if name == "b" else (renderers["default"], osc)
    out = torch.full((H, W, 3), SENTINEL, dtype=torch.float32, device="cuda")
    with r.accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
        assert acc.has_points and not acc.has_rays and acc.view is None and acc.samples == 0
        done, traced, fallbacks = 0, 0, 0
        for k in SPLIT:
            st = acc.add(k, out.data_ptr())
            done += k
            mean, traces = _ref(o_sc, sets, name, integrator, done)
            assert acc.samples == done and st["samples"] == W * H * k, done
            assert st["rays_reference"] == traces - traced, done
            assert st["work_units"] >= W * H
            traced = traces
            fallbacks += st["accel_fallbacks"]
            _check(acc, mean)
        one_shot, ost = r.render_irradiance(p, n, W, H, done, BOUNCES, integrator, SEED)
        torch.cuda.synchronize()
        assert _bits(out.cpu().numpy()) == _bits(one_shot)                       # d_out of the last pass
        assert _bits(acc.image()) == _bits(one_shot) and ost["rays_reference"] == traced
        assert np.count_nonzero(one_shot) > W * H // 4
        if name == "d":
            assert fallbacks > 0                                               # the 2^-60 coordinates took the exact culled walk
    if integrator == 0:                                                        # every trace() of the loop, and no other
        with r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED, NDPS) as acc:
            assert sum(acc.add(k)["rays_traced"] for k in SPLIT) == _ref(o_sc, sets, name, 0, 4)[1]
            _check(acc, _ref(o_sc, sets, name, 0, 4)[0])


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_split_units(renderers, osc, sets, name, integrator):
    """PT_WF_CHUNKS=3: split units, whose replay skips a pair and the integrator's draws per earlier sample, from a
    stream that continues the first pass's; PT_WF_CHUNKS=1: whole-pixel units."""
    p, n = sets[name]
    m3, t3 = _ref(osc, sets, name, integrator, 3)
    m7, t7 = _ref(osc, sets, name, integrator, 7)
    for which in ("chunks", "whole"):
        with renderers[which].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
            s3 = acc.add(3)
            _check(acc, m3)
            s4 = acc.add(4)
            _check(acc, m7)
            assert s3["rays_reference"] == t3 and s4["rays_reference"] == t7 - t3
            if which == "chunks":
                assert s3["split_pixels"] > 0 and s4["split_pixels"] > 0 and s4["work_units"] > W * H
            else:
                assert s3["split_pixels"] == 0 and s4["split_pixels"] == 0 and s4["work_units"] == W * H


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "c"])
def test_flags(renderers, osc, sets, name, integrator):
    p, n = sets[name]
    mean, _ = _ref(osc, sets, name, integrator, 4)
    for which in ("default", "whole"):
        traced = {}
        for flags in (0, NPC, NDPS, NPC | NDPS):
            with renderers[which].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED, flags) as acc:
                traced[flags] = sum(acc.add(k)["rays_traced"] for k in SPLIT)
                _check(acc, mean)
        # no sample-invariant ray, no memo: PT_FLAG_NO_PRIMARY_CACHE changes neither the image nor what is traced
        assert traced[NPC] == traced[0] and traced[NPC | NDPS] == traced[NDPS]


# ---- 2. what create refuses
def test_irregular_and_invalid_points_are_refused(renderers, sets):
    r = renderers["default"]
    p, n = sets["e"]
    with pytest.raises(pt.PtError) as e:
        r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED)
    assert e.value.code == pt.PT_E_INVALID and "1 irregular" in str(e.value) and "pt_render_irradiance" in str(e.value)
    dp = _dev(p, n)
    with pytest.raises(pt.PtError) as e:
        r.accumulator_points_device(dp.data_ptr(), W, H, BOUNCES, 1, SEED)
    assert e.value.code == pt.PT_E_INVALID and "1 irregular" in str(e.value)
    # invalid points: a zero, a NaN and a 1.01-long normal and an infinite position -- the lowest such pixel is named,
    # also when it lies outside this shard's pixels
    p, n = sets["a"]
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
        for make in (lambda: r.accumulator_points(p2, n2, W, H, BOUNCES, 0, SEED),
                     lambda: r.accumulator_points_device(bad.data_ptr(), W, H, BOUNCES, 1, SEED, shard_index=1, shard_count=2)):
            with pytest.raises(pt.PtError) as e:
                make()
            assert e.value.code == pt.PT_E_INVALID and "invalid points" in str(e.value), str(e.value)
            assert "pixel (%d, %d)" % (at % W, at // W) in str(e.value), str(e.value)
    m = 16
    mp, mn = iref.set_floor(m, m)
    mp, mn = iref.to_morton(mp, m), iref.to_morton(mn, m)
    mn[iref.morton(5, 9)] = 0
    with pytest.raises(pt.PtError) as e:
        r.accumulator_points(mp, mn, m, m, pixel_order=pt.PT_ORDER_MORTON)
    assert e.value.code == pt.PT_E_INVALID and "pixel (5, 9)" in str(e.value)
    # a misaligned device buffer, a null one
    good = _dev(p, n)
    with pytest.raises(pt.PtError) as e:
        r.accumulator_points_device(good.data_ptr() + 4, W, H - 1)
    assert e.value.code == pt.PT_E_INVALID and "aligned" in str(e.value)
    with pytest.raises(pt.PtError) as e:
        r.accumulator_points_device(0, W, H)
    assert e.value.code == pt.PT_E_INVALID and "null" in str(e.value)
    # the context still renders
    img, _ = r.render_irradiance(p, n, W, H, 2, BOUNCES, 0, SEED)
    assert np.count_nonzero(img) > 0


def test_flags_occupancy_and_saves_are_refused(renderers, scene, sets, tmp_path):
    r = renderers["default"]
    p, n = sets["a"]
    for flags in (pt.PT_FLAG_JITTER, pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT, pt.PT_FLAG_JITTER_TENT, pt.PT_FLAG_COUNT,
                  pt.PT_FLAG_COUNT | pt.PT_FLAG_TRI_COUNTS, pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH, 0x100,
                  NPC | pt.PT_FLAG_JITTER):
        with pytest.raises(pt.PtError) as e:
            r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED, flags)
        assert e.value.code == pt.PT_E_INVALID and "flags" in str(e.value), hex(flags)
    for env, integrator in (({"PT_WF_MIN_WAVES": "4"}, 0), ({"PT_HEAD_MIN_WAVES": "4"}, 1), ({"PT_HEAD_WF": "0"}, 1)):
        r2 = _renderer(scene, env)
        try:
            with pytest.raises(pt.PtError) as e:
                r2.accumulator_points(p, n, W, H, BOUNCES, integrator, SEED)
            assert e.value.code == pt.PT_E_INVALID and ("MIN_WAVES" in str(e.value) or "PT_HEAD_WF" in str(e.value))
        finally:
            r2.close()
    with r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED) as acc, acc.noise() as est:
        acc.add(2)
        est.update()
        for save in (lambda: acc.save(str(tmp_path / "x.ptacc")), lambda: acc.save_session(str(tmp_path / "x.ptses")),
                     lambda: acc.save_session(str(tmp_path / "y.ptses"), est)):
            with pytest.raises(pt.PtError) as e:
                save()
            assert e.value.code == pt.PT_E_INVALID and "point" in str(e.value)
        assert not os.listdir(str(tmp_path))
    # a render in flight
    buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    r.render_device_async(_cam(), buf.data_ptr(), W, H, 2, BOUNCES, 0, SEED)
    try:
        with pytest.raises(pt.PtError) as e:
            r.accumulator_points(p, n, W, H)
        assert e.value.code == pt.PT_E_INVALID and "in flight" in str(e.value)
    finally:
        r.wait()


def test_has_points_has_rays_and_view(renderers, sets):
    r = renderers["default"]
    p, n = sets["a"]
    with r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED) as acc:
        assert acc.has_points is True and acc.has_rays is False and acc.view is None
    with r.accumulator(_cam(), W, H, BOUNCES, 0, SEED) as acc:
        assert acc.has_points is False and acc.has_rays is False
    o, d = rays.ortho_rays((0.0, 1.0, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.8, 1.8, W, H)
    with r.accumulator_rays(o, d, W, H, BOUNCES, 0, SEED) as acc:
        assert acc.has_points is False and acc.has_rays is True


# ---- 3. ownership: the accumulator keeps its own copy of the points
@pytest.mark.parametrize("integrator", [0, 1])
def test_the_callers_buffer_may_be_overwritten(renderers, osc, sets, integrator):
    r = renderers["default"]
    p, n = sets["c"]
    dp = _dev(p, n)
    with r.accumulator_points_device(dp.data_ptr(), W, H, BOUNCES, integrator, SEED) as acc:
        dp.fill_(float("nan"))
        torch.cuda.synchronize()
        done = 0
        for k in SPLIT:
            acc.add(k)
            done += k
            _check(acc, _ref(osc, sets, "c", integrator, done)[0])
    # on a stream of the caller's
    dp = _dev(p, n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        acc = r.accumulator_points_device(dp.data_ptr(), W, H, BOUNCES, integrator, SEED, stream_ptr=s.cuda_stream)
        dp.fill_(float("nan"))
    torch.cuda.synchronize()
    with acc:
        acc.add(4)
        _check(acc, _ref(osc, sets, "c", integrator, 4)[0])


# ---- 4. geometry
@pytest.fixture(scope="module")
def frame37(renderers, osc):
    w, h = 37, 19
    p, n, _ = rays.feature_points(renderers["default"].features(_cam(w, h), w, h), iref.LIFT)
    refs = {i: np.asarray(iref.render(osc, p, n, w, h, 4, BOUNCES, i, SEED)) for i in (0, 1)}
    return w, h, p, n, refs


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("count,tile", [(2, (0, 0)), (3, (16, 8))])
def test_shards_sum_to_the_frame(renderers, frame37, count, tile, integrator):
    w, h, p, n, refs = frame37
    ref = refs[integrator]
    r = renderers["default"]
    total = np.zeros_like(ref)
    for k in range(count):
        with r.accumulator_points(p, n, w, h, BOUNCES, integrator, SEED, shard_index=k, shard_count=count, tile=tile) as acc:
            mine = shard.shard_pixels_lib(w, h, k, count, tile[0], tile[1])
            assert acc.add(2)["samples"] == len(mine) * 2 and acc.add(2)["samples"] == len(mine) * 2
            want = np.zeros_like(ref)
            want.reshape(-1, 3)[mine] = ref.reshape(-1, 3)[mine]
            _check(acc, want)                                  # (pixels outside the shard read as 0)
            assert 0 < len(mine) < w * h
            assert _bits(acc.active_pixels()) == _bits(mine)
            total += acc.mean64()
    assert _bits(total) == _bits(ref)


@pytest.mark.parametrize("integrator", [0, 1])
def test_partial_tiles_and_an_empty_shard(renderers, frame37, integrator):
    w, h, p, n, refs = frame37
    r = renderers["default"]
    with r.accumulator_points(p, n, w, h, BOUNCES, integrator, SEED, tile=(16, 24)) as acc:   # partial tiles right and below
        acc.add(3)
        acc.add(1)
        _check(acc, refs[integrator])
    out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
    with r.accumulator_points(p, n, w, h, BOUNCES, integrator, SEED, shard_index=7, shard_count=8, tile=256) as acc:
        st = acc.add(4, out.data_ptr())
        torch.cuda.synchronize()
        assert st["samples"] == 0 and st["rays_traced"] == 0 and st["rays_reference"] == 0 and st["work_units"] == 0
        assert acc.samples == 4
        assert (out.cpu().numpy() == F(SENTINEL)).all()
        assert not acc.mean64().any() and acc.active_pixels().size == 0 and not acc.counts().any()


@pytest.mark.parametrize("integrator", [0, 1])
def test_morton_order(renderers, osc, integrator):
    m = 16
    p, n, _ = rays.feature_points(renderers["default"].features(_cam(m, m), m, m), iref.LIFT)
    ref = np.asarray(iref.render(osc, p, n, m, m, 3, BOUNCES, integrator, SEED))
    with renderers["default"].accumulator_points(iref.to_morton(p, m), iref.to_morton(n, m), m, m, BOUNCES, integrator, SEED,
                                                 pixel_order=pt.PT_ORDER_MORTON) as acc:
        acc.add(1)
        acc.add(2)
        assert acc.mean64().shape == (m * m, 3)
        _check(acc, iref.to_morton(ref.reshape(-1, 3), m))
    # (scanline points under a Morton accumulator would be other pixels' points)
    with renderers["default"].accumulator_points(p, n, m, m, BOUNCES, integrator, SEED, pixel_order=pt.PT_ORDER_MORTON) as acc:
        acc.add(3)
        assert _bits(acc.mean64()) != _bits(iref.to_morton(ref.reshape(-1, 3), m))


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("size", [(100, 1), (1, 1)])
def test_thin_images(renderers, osc, size, integrator):
    w, h = size
    p, n = rays.grid_points((-0.9, 0.0, 0.3), (0.0, 0.0, 0.1), (1.8, 0.0, 0.0), w, h, iref.LIFT)
    ref = np.asarray(iref.render(osc, p, n, w, h, 4, BOUNCES, integrator, SEED))
    ref2 = np.asarray(iref.render(osc, p, n, w, h, 2, BOUNCES, integrator, SEED))
    if size == (100, 1):
        assert np.count_nonzero(ref) > 0
    for which in ("default", "chunks"):
        with renderers[which].accumulator_points(p, n, w, h, BOUNCES, integrator, SEED) as acc:
            acc.add(2)
            acc.add(2)
            _check(acc, ref)
        with renderers[which].accumulator_points(p, n, w, h, BOUNCES, integrator, SEED) as acc:   # and over the active list
            acc.add(2)
            mask = np.zeros((h, w), dtype=bool)
            mask[0, ::3] = w > 1
            acc.freeze(mask)
            acc.add(2)
            _check(acc, np.where(mask[..., None], ref2, ref))


# ---- 5. masked and frozen texels
@pytest.mark.parametrize("integrator", [0, 1])
def test_masked_texels_of_a_chart(renderers, scene, osc, integrator):
    """pt_accum_freeze at 0 samples over ~covered of a chart laid on the floor: those texels stay at mean 0 and count 0
    and are never sampled; every other texel is the restatement's."""
    tris, uvs = iar.floor_chart(scene.arrays())
    p, n, tri, covered = chart_points(scene.arrays(), tris, uvs, W, H, iref.LIFT)
    assert 0 < covered.sum() < W * H and (tri[~covered] == -1).all()
    mask = ~covered.reshape(H, W)
    mean = np.asarray(iref.render_cached("cornell/chart", osc, p, n, W, H, 4, BOUNCES, integrator, SEED)[0])
    assert np.count_nonzero(mean[~mask]) > 0
    every = shard.shard_pixels_lib(W, H, 0, 1)
    for which in ("default", "chunks"):
        with renderers[which].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
            acc.freeze(mask)
            assert _bits(acc.active_pixels()) == _bits(every[~mask.reshape(-1)[every]])
            for k in SPLIT:
                st = acc.add(k)
                assert st["samples"] == int((~mask).sum()) * k and st["work_units"] == int((~mask).sum())
            _check(acc, np.where(mask[..., None], 0.0, mean))
            assert _bits(acc.counts()) == _bits(np.where(mask, 0, 4).astype(np.uint32))
            assert _bits(acc.active_pixels()) == _bits(every[~mask.reshape(-1)[every]])


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("name", ["a", "d"])
def test_texels_frozen_at_two_samples(renderers, osc, sets, name, integrator):
    """Passes 2, freeze a checkerboard, 2 more: the second pass runs over the active list (init_active_states_points),
    the frozen texels keep their 2-sample value and the others reach the 4-sample one."""
    p, n = sets[name]
    mask = iar.checkerboard(W, H, 3)
    render = iar.means(osc, name, p, n, integrator)
    t2, t4 = (_ref(osc, sets, name, integrator, k)[1] for k in (2, 4))
    want, counts = iar.frozen_at(render, mask, 2, 4)
    every = shard.shard_pixels_lib(W, H, 0, 1)
    for which in ("default", "chunks", "whole"):
        with renderers[which].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
            assert acc.add(2)["rays_reference"] == t2
            acc.freeze(mask)
            st = acc.add(2)
            assert st["samples"] == int((~mask).sum()) * 2 and 0 < st["rays_reference"] < t4 - t2
            _check(acc, want)
            assert _bits(acc.counts()) == _bits(counts)
            assert _bits(acc.active_pixels()) == _bits(every[~mask.reshape(-1)[every]])
            acc.freeze(np.ones((H, W), dtype=bool))            # everything frozen: a pass samples nothing
            st = acc.add(3)
            assert st["samples"] == 0 and acc.active_pixels().size == 0
            _check(acc, want)
    # two passes of 1 over the active list, from the stream the first of them left
    with renderers["default"].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
        acc.add(2)
        acc.freeze(mask)
        acc.add(1)
        acc.add(1)
        _check(acc, want)


# ---- 6. the noise estimator, fed with the restatement's means
@pytest.mark.parametrize("integrator", [0, 1])
def test_noise_estimates(renderers, osc, sets, integrator):
    p, n = sets["c"]
    ref = noise_ref.NoiseRef(0, shape=(H, W))
    with renderers["default"].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc, acc.noise() as est:
        done = 0
        for k in SPLIT:
            acc.add(k)
            done += k
            assert ref.update(done, _ref(osc, sets, "c", integrator, done)[0])
            for tol in (0.05, 0.25, 1.0):
                s = est.update(tol=tol)
                want = ref.summary(tol, noise_ref.Y_FLOOR)
                assert s["samples"] == done and {k2: s[k2] for k2 in want} == want, (done, tol)
            mu, m2 = est.read()
            assert _bits(mu) == _bits(ref.mu) and _bits(m2) == _bits(ref.m2)
            assert _bits(est.error_map()) == _bits(ref.error_map(noise_ref.Y_FLOOR))
            assert _bits(est.variance()) == _bits(denoise_guided_ref.variance_ref(ref, done))
        assert s["pixels"] == W * H and s["batches"] == len(SPLIT)


# ---- 7. the loops, on the case whose condition tests/test_irradiance_accum_host.py checks
@pytest.mark.parametrize("integrator", [0, 1])
def test_add_adaptive(renderers, osc, sets, integrator):
    LOOP = iar.LOOP
    p, n = sets[iar.LOOP_SET]
    render = iar.means(osc, iar.LOOP_SET, p, n, integrator)
    sim = adaptive_ref.simulate(render, (H, W), **LOOP)
    kw = dict(tol=LOOP["tol"], quantile=LOOP["quantile"], min_batches=LOOP["min_batches"])
    every = shard.shard_pixels_lib(W, H, 0, 1)
    with renderers["default"].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
        res = acc.add_adaptive(LOOP["pass_spp"], LOOP["cap"], **kw)
        counts, mean, state = acc.counts(), acc.mean64(), acc._noise.read()
        emap, var, active = acc._noise.error_map(), acc._noise.variance(), acc.active_pixels()
        assert _bits(acc.image()) == _bits(mean.astype(F))
    print("integrator %d: samples_total %d of %d, active %d" % (integrator, res["samples_total"], W * H * LOOP["cap"], res["active"]))
    assert _bits(counts) == _bits(sim["counts"]) and res["samples_total"] == sim["samples_total"] == int(counts.sum())
    assert res["passes"] == sim["passes"] and res["stopped_converged"] == sim["stopped_converged"]
    assert res["samples"] == int(counts.max()) and 0 < res["active"] == sim["active"] < W * H
    frozen_n = W * H - res["active"]
    assert W * H // 10 <= frozen_n <= (W * H * 9) // 10                          # (the host test's condition)
    assert len(set(np.unique(counts)) - {LOOP["cap"]}) >= 2
    want = sim["summary"]
    assert {k: res["summary"][k] for k in want} == want
    assert _bits(mean) == _bits(adaptive_ref.compose(render, counts))
    assert _bits(state[0]) == _bits(sim["est"].mu) and _bits(state[1]) == _bits(sim["est"].m2)
    assert _bits(emap) == _bits(sim["est"].error_map())
    assert _bits(var) == _bits(denoise_guided_ref.variance_ref(sim["est"], counts))
    # the active list: the loop's last step froze what had converged by then
    frozen = (counts < counts.max()) | sim["est"].converged(LOOP["tol"])
    assert int((~frozen).sum()) == sim["active"]
    assert _bits(active) == _bits(every[~frozen.reshape(-1)[every]])


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("quantile", [0.5, 1.0])
def test_add_until(renderers, osc, sets, integrator, quantile):
    LOOP = iar.LOOP
    p, n = sets[iar.LOOP_SET]
    render = iar.means(osc, iar.LOOP_SET, p, n, integrator)
    # pt_accum_add_until restated over noise_ref
    ref = noise_ref.NoiseRef(0, shape=(H, W))
    samples, passes, stopped, summ = 0, 0, False, None
    while samples < LOOP["cap"]:
        samples += min(LOOP["pass_spp"], LOOP["cap"] - samples)
        ref.update(samples, render(samples))
        passes += 1
        summ = ref.summary(LOOP["tol"], noise_ref.Y_FLOOR)
        if summ["batches"] >= LOOP["min_batches"] and summ["converged"] >= int(np.ceil(np.float64(F(quantile)) * summ["pixels"])):
            stopped = True
            break
    with renderers["default"].accumulator_points(p, n, W, H, BOUNCES, integrator, SEED) as acc:
        res = acc.add_until(LOOP["pass_spp"], LOOP["cap"], tol=LOOP["tol"], quantile=quantile, min_batches=LOOP["min_batches"])
        print("quantile %g: passes %d, stopped %s, samples %d" % (quantile, res["passes"], res["stopped_converged"], res["samples"]))
        assert (res["passes"], res["stopped_converged"], res["samples"]) == (passes, stopped, samples)
        assert {k: res["summary"][k] for k in summ} == summ
        _check(acc, render(samples))
        mu, m2 = acc._noise.read()
        assert _bits(mu) == _bits(ref.mu) and _bits(m2) == _bits(ref.m2)
        assert _bits(acc._noise.error_map()) == _bits(ref.error_map(noise_ref.Y_FLOOR))
        assert _bits(acc._noise.variance()) == _bits(denoise_guided_ref.variance_ref(ref, samples))
        assert (acc.counts() == samples).all() and acc.active_pixels().size == W * H


# ---- 8. a scene with spheres and nine lights (more than the kLdsLights = 5 staged in LDS), two of them spheres
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
    ref2, c2 = iref.render(o_sc, p, n, W, H, 2, BOUNCES, 0, SEED, return_counters=True)
    ref4, c4 = iref.render(o_sc, p, n, W, H, 4, BOUNCES, 0, SEED, return_counters=True)
    assert np.count_nonzero(ref4) > 0
    with pt.Renderer(s, 0) as r, r.accumulator_points(p, n, W, H, BOUNCES, 0, SEED) as acc:
        st = acc.add(2)
        assert st["rays_reference"] == c2["traces"] and st["work_units"] > 0
        _check(acc, np.asarray(ref2))
        st = acc.add(2)
        assert st["rays_reference"] == c4["traces"] - c2["traces"]
        _check(acc, np.asarray(ref4))
