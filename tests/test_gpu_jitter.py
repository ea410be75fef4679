"""Sub-pixel jitter on the GPU (include/pt/pt.h, PT_FLAG_JITTER / PT_FLAG_JITTER_TENT): every render path with the
flag equals jitter_ref -- the oracle's per-pixel loop restated around the numpy restatement of the jittered ray, the
two film-point draws first in every sample -- in every bit.  Cornell box, 24 x 16, 4 samples, 3 bounces, seed 1234
unless said otherwise; a full frame includes Morton index 0, the reference's quirk lens pixel."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import shard
from cudapathtracer_amd import jitter_offset                 # (the parent has no such name: every test here errors there)
import jitter_ref
import light_scenes as ls
import oracle
import view_ref

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, SPP, BOUNCES, SEED = 24, 16, 4, 3, 1234
POS = (0.0, 1.0, 3.0)
VIEWS = {"null": None, "generic": view_ref.generic(POS)}
KINDS = {"box": pt.PT_FLAG_JITTER, "tent": pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT}
RT, RB, CNT, NPC = pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH, pt.PT_FLAG_COUNT, pt.PT_FLAG_NO_PRIMARY_CACHE


def _view(name):
    v = VIEWS[name]
    return None if v is None else pt.make_view(v[0], v[1], v[2], v[3])


def _cam(radius, w=W, h=H, pos=POS, dist=1.0, focal=3.0):
    return pt.make_camera(pos, dist, focal, radius, w, h)


def _rcam(radius, w=W, h=H, pos=POS, dist=1.0, focal=3.0):
    return (tuple(pos), dist, focal, radius, w, h)


@pytest.fixture(scope="module")
def scene():
    return load_scene("cornell")


@pytest.fixture(scope="module")
def osc(scene):
    return oracle.OracleScene(scene.arrays())


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
def renderers(scene):
    rs = {"default": _renderer(scene, {}), "tile_head": _renderer(scene, {"PT_HEAD_WF": "0"}),
          "chunks": _renderer(scene, {"PT_WF_CHUNKS": "3"})}
    yield rs
    for r in rs.values():
        r.close()


def _ref(osc, kind, view, radius, integrator, spp=SPP, w=W, h=H, counters=False):
    """The restated image of the Cornell box (shared, read-only); kind None: the unjittered one."""
    flags = KINDS[kind] if kind else 0
    return jitter_ref.render_cached("cornell", osc, _rcam(radius, w, h), VIEWS[view], flags, spp, BOUNCES, integrator, SEED,
                                    return_counters=counters)


def _same(img, ref64):
    return jitter_ref.same_bits(img, np.asarray(ref64).astype(F))


# ---- the render paths: the three kernel families
PATHS = {
    "wavefront_unidir": ("default", 0, 0),
    "wavefront_head": ("default", 1, 0),
    "tile_reference_walk_unidir": ("default", 0, RT),
    "tile_reference_walk_head": ("default", 1, RT),
    "tile_head_wf_off": ("tile_head", 1, 0),
}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_jittered_render(renderers, osc, kind, view, radius, path):
    which, integrator, flags = PATHS[path]
    img, st = renderers[which].render(_cam(radius), W, H, SPP, BOUNCES, integrator, SEED, flags | KINDS[kind], view=_view(view))
    ref, cnt = _ref(osc, kind, view, radius, integrator, counters=True)
    print("%s %s %s r=%g: differing %d, samples %d, rays_reference %d (restatement %d), rays_traced %d, work_units %d"
          % (path, kind, view, radius, _same(img, ref), st["samples"], st["rays_reference"], cnt["traces"], st["rays_traced"],
             st["work_units"]))
    assert st["samples"] == W * H * SPP
    assert (st["work_units"] > 0) == path.startswith("wavefront")      # the kernel family the case is about
    assert st["rays_reference"] == cnt["traces"]
    assert _same(img, ref) == 0, (kind, view, radius, path)
    assert np.count_nonzero(ref) > W * H                               # (the shot sees the scene)


# ---- every kernel instance a jittered render can run.  The Cornell box fits the LDS tree, so the default renderer runs
# the LDS-walk instances; PT_WF_LDS_TREE=0 gives the others.  (env, integrator, flags, wavefront)
INSTANCES = {
    "unidir_lds_walk": ({}, 0, 0, True),
    "unidir_memory_walk": ({"PT_WF_LDS_TREE": "0"}, 0, 0, True),
    "unidir_count_lds_walk": ({}, 0, CNT, True),
    "unidir_count_memory_walk": ({"PT_WF_LDS_TREE": "0"}, 0, CNT, True),
    "unidir_count_min_waves_4": ({"PT_WF_MIN_WAVES": "4"}, 0, CNT, True),
    "unidir_min_waves_4": ({"PT_WF_MIN_WAVES": "4"}, 0, 0, True),
    "unidir_min_waves_6": ({"PT_WF_MIN_WAVES": "6"}, 0, 0, True),
    "head": ({}, 1, 0, True),
    "head_count": ({}, 1, CNT, True),
    "head_min_waves_4": ({"PT_HEAD_MIN_WAVES": "4"}, 1, 0, True),
    "tile_unidir_reference_bvh": ({}, 0, RB, False),
    "tile_unidir_reference_bvh_count": ({}, 0, RB | CNT, False),
    "tile_head_reference_bvh": ({}, 1, RB, False),
    "tile_head_reference_bvh_count": ({}, 1, RB | CNT, False),
    "tile_head_fast4": ({"PT_HEAD_WF": "0"}, 1, 0, False),
    "tile_head_fast4_count": ({"PT_HEAD_WF": "0"}, 1, CNT, False),
    "tile_head_fast4_off": ({"PT_HEAD_WF": "0", "PT_TILE_FAST4": "0"}, 1, 0, False),
    "tile_unidir_reference_walk_count": ({}, 0, RT | CNT, False),
    "tile_head_reference_walk_count": ({}, 1, RT | CNT, False),
}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_every_jittered_kernel_instance(scene, osc, name):
    env, integrator, flags, wavefront = INSTANCES[name]
    r = _renderer(scene, env)
    try:
        for kind, view, radius in (("box", "null", 0.0), ("tent", "generic", 0.05)):
            ref = _ref(osc, kind, view, radius, integrator)
            img, st = r.render(_cam(radius), W, H, SPP, BOUNCES, integrator, SEED, flags | KINDS[kind], view=_view(view))
            assert (st["work_units"] > 0) == wavefront and st["samples"] == W * H * SPP, (name, kind)
            assert _same(img, ref) == 0, (name, kind, view, radius)
            if flags & CNT:
                assert st["node_tests"] > 0
            if name in ("unidir_lds_walk", "unidir_memory_walk", "head"):      # the accumulating twins
                with r.accumulator(_cam(radius), W, H, BOUNCES, integrator, SEED, KINDS[kind], view=_view(view)) as acc:
                    acc.add(1)
                    acc.add(3)
                    assert _same(acc.image(), ref) == 0, (name, kind, view, radius)
    finally:
        r.close()


# ---- split units: a pixel's later chunks start from a stream replayed over the earlier samples -- two more draws per
# sample (and 7 + 2 + 2 for integrator 1); one wrong count shifts every later sample
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_split_units(renderers, osc, radius, integrator):
    for kind, view, spp in (("box", "null", SPP), ("tent", "generic", SPP), ("box", "null", 7)):
        img, st = renderers["chunks"].render(_cam(radius), W, H, spp, BOUNCES, integrator, SEED, KINDS[kind], view=_view(view))
        assert st["split_pixels"] > 0 and st["samples"] == W * H * spp
        assert _same(img, _ref(osc, kind, view, radius, integrator, spp=spp)) == 0, (kind, view, spp)
    with renderers["chunks"].accumulator(_cam(radius), W, H, BOUNCES, integrator, SEED, KINDS["box"]) as acc:
        st1 = acc.add(3)
        st2 = acc.add(4)
        assert st1["split_pixels"] > 0 and st2["split_pixels"] > 0
        assert _same(acc.image(), _ref(osc, "box", "null", radius, integrator, spp=7)) == 0


# ---- accumulators
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_accumulator(scene, renderers, osc, tmp_path, radius, integrator):
    r = renderers["default"]
    flags = KINDS["tent"]
    ref = _ref(osc, "tent", "null", radius, integrator)
    f = str(tmp_path / "c.ptacc")
    with r.accumulator(_cam(radius), W, H, BOUNCES, integrator, SEED, flags) as acc:
        acc.add(1)
        acc.add(3)
        assert _same(acc.image(), ref) == 0
    with r.accumulator(_cam(radius), W, H, BOUNCES, integrator, SEED, flags) as acc:
        acc.add(2)
        acc.save(f)
    assert pt.accum_file_info(f)["params"].flags == flags
    fresh = _renderer(scene, {})
    try:
        with fresh.load_accumulator(f) as acc:
            assert acc.samples == 2 and acc.params.flags == flags
            acc.add(2)
            assert _same(acc.image(), ref) == 0
            # freeze half of the pixels (not pixel 0, the quirk lens pixel): the adaptive set-up samples the rest
            mask = np.zeros((H, W), dtype=np.uint8)
            mask[::2, 1::2] = 1
            mask[1::2, ::2] = 1
            acc.freeze(mask)
            acc.add(2)
            counts = acc.counts()
            assert np.array_equal(counts, np.where(mask != 0, 4, 6))
            want = jitter_ref.render(osc, _rcam(radius), None, flags, 0, BOUNCES, integrator, SEED, counts=counts)
            assert jitter_ref.same_bits(acc.mean64(), want) == 0
    finally:
        fresh.close()


def test_session_file_with_a_view_and_frozen_pixels(scene, renderers, osc, tmp_path):
    r = renderers["default"]
    flags, radius = KINDS["box"], 0.05
    f = str(tmp_path / "s.ptses")
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[:, W // 2:] = 1
    with r.accumulator(_cam(radius), W, H, BOUNCES, 0, SEED, flags, view=_view("generic")) as acc:
        acc.add(2)
        acc.freeze(mask)
        acc.save_session(f)
    assert pt.session_file_info(f)["params"].flags == flags and pt.session_file_view(f) is not None
    fresh = _renderer(scene, {})
    try:
        acc, _ = fresh.load_session(f)
        with acc:
            assert acc.params.flags == flags and acc.view is not None
            acc.add(2)
            counts = acc.counts()
            assert np.array_equal(counts, np.where(mask != 0, 2, 4))
            want = jitter_ref.render(osc, _rcam(radius), VIEWS["generic"], flags, 0, BOUNCES, 0, SEED, counts=counts)
            assert jitter_ref.same_bits(acc.mean64(), want) == 0
            left = np.asarray(_ref(osc, "box", "generic", radius, 0)).astype(F)[:, :W // 2]
            assert jitter_ref.same_bits(acc.image()[:, :W // 2], left) == 0      # the unfrozen half: the one-shot render
    finally:
        fresh.close()


@pytest.mark.parametrize("integrator", [0, 1])
def test_add_adaptive(renderers, osc, integrator):
    flags = KINDS["box"]
    with renderers["default"].accumulator(_cam(0.0), W, H, BOUNCES, integrator, SEED, flags) as acc:
        res = acc.add_adaptive(2, 8, tol=0.2)
        counts = acc.counts()
        print("add_adaptive i=%d: passes %d, counts %s" % (integrator, res["passes"], np.unique(counts, return_counts=True)))
        assert res["passes"] >= 2 and counts.max() <= 8 and counts.min() >= 2
        want = jitter_ref.render(osc, _rcam(0.0), None, flags, 0, BOUNCES, integrator, SEED, counts=counts)
        assert jitter_ref.same_bits(acc.mean64(), want) == 0


# ---- shards and pixel orders
def test_three_shards_sum_to_the_frame(renderers, osc):
    w, h = 37, 19
    r = renderers["default"]
    flags = KINDS["tent"]
    ref = np.asarray(jitter_ref.render_cached("cornell", osc, _rcam(0.05, w, h), None, flags, SPP, BOUNCES, 0, SEED)).astype(F)
    total = np.zeros_like(ref)
    owned = np.zeros(w * h, dtype=np.int32)
    for k in range(3):
        img, st = r.render(_cam(0.05, w, h), w, h, SPP, BOUNCES, 0, SEED, flags, shard_index=k, shard_count=3, tile_w=16, tile_h=8)
        mine = shard.shard_pixels(w, h, k, 3, 16, 8)
        owned[mine] += 1
        assert 0 < len(mine) < w * h and st["samples"] == len(mine) * SPP
        want = np.zeros_like(ref)
        want.reshape(-1, 3)[mine] = ref.reshape(-1, 3)[mine]
        assert jitter_ref.same_bits(img, want) == 0, k
        total += img
    assert (owned == 1).all() and jitter_ref.same_bits(total, ref) == 0
    # a shard that owns no pixel: nothing is launched, the image stays zero
    img, st = r.render(_cam(0.05, w, h), w, h, SPP, BOUNCES, 0, SEED, flags, shard_index=7, shard_count=8, tile_w=256, tile_h=256)
    assert st["samples"] == 0 and not img.any()


def test_morton_order(renderers, osc):
    n = 16
    flags = KINDS["box"]
    ref = jitter_ref.render_cached("cornell", osc, _rcam(0.0, n, n), None, flags, 3, BOUNCES, 0, SEED).astype(F)
    img, _ = renderers["default"].render(_cam(0.0, n, n), n, n, 3, BOUNCES, 0, SEED, flags, pixel_order=pt.PT_ORDER_MORTON)
    want = np.zeros((n * n, 3), dtype=F)
    for y in range(n):
        for x in range(n):
            want[view_ref.morton(x, y)] = ref[y, x]
    assert jitter_ref.same_bits(img, want) == 0


# ---- not ignored and not leaking
def _differing_pixels(a, b):
    return int(np.count_nonzero(np.any(np.asarray(a) != np.asarray(b), axis=2)))


def test_jitter_is_not_ignored_and_does_not_leak(renderers, osc):
    """On each kernel family a jittered image differs from the plain one in more than half of the frame's pixels, and
    a plain render taken after a jittered one on the same context is the plain render."""
    for which, integrator, flags in ((w, i, f) for w, i, f in sorted(PATHS.values())):
        r = renderers[which]
        plain0, _ = r.render(_cam(0.0), W, H, SPP, BOUNCES, integrator, SEED, flags)
        jit, _ = r.render(_cam(0.0), W, H, SPP, BOUNCES, integrator, SEED, flags | KINDS["box"])
        tent, _ = r.render(_cam(0.0), W, H, SPP, BOUNCES, integrator, SEED, flags | KINDS["tent"])
        plain1, _ = r.render(_cam(0.0), W, H, SPP, BOUNCES, integrator, SEED, flags)
        assert _differing_pixels(jit, plain0) > W * H // 2 and _differing_pixels(jit, tent) > W * H // 2
        assert jitter_ref.same_bits(plain0, plain1) == 0
        assert _same(plain1, _ref(osc, None, "null", 0.0, integrator)) == 0
        # PT_FLAG_NO_PRIMARY_CACHE on top of jitter changes no bit
        npc, st = r.render(_cam(0.0), W, H, SPP, BOUNCES, integrator, SEED, flags | KINDS["box"] | NPC)
        assert jitter_ref.same_bits(npc, jit) == 0


def test_tent_alone_is_refused(renderers):
    r = renderers["default"]
    for call in (lambda: r.render(_cam(0.0), W, H, 1, flags=pt.PT_FLAG_JITTER_TENT),
                 lambda: r.accumulator(_cam(0.0), W, H, flags=pt.PT_FLAG_JITTER_TENT),
                 lambda: r.features(_cam(0.0), W, H, flags=pt.PT_FLAG_JITTER_TENT)):
        with pytest.raises(pt.PtError) as e:
            call()
        assert e.value.code == pt.PT_E_INVALID and "PT_FLAG_JITTER_TENT" in str(e.value)


@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
def test_async_renders_with_different_flags(renderers, osc, two_streams):
    """Two renders in flight, one jittered and one plain (then tent and box, the other integrator second): each frame
    equals its own reference.  Repeated, so that both flight slots are reused with the other flags."""
    import torch
    r = renderers["default"]
    rounds = [[("box", 0), (None, 1)], [(None, 0), ("tent", 1)]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two_streams else [torch.cuda.Stream()] * 2
    bufs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    for order in rounds:
        for k, (kind, integ) in enumerate(order):
            s = streams[k]
            with torch.cuda.stream(s):
                bufs[k].zero_()
                r.render_device_async(_cam(0.05), bufs[k].data_ptr(), W, H, SPP, BOUNCES, integ, SEED,
                                      KINDS[kind] if kind else 0, stream_ptr=s.cuda_stream)
        stats = [r.wait(), r.wait()]
        torch.cuda.synchronize()
        for k, (kind, integ) in enumerate(order):
            assert _same(bufs[k].cpu().numpy(), _ref(osc, kind, "null", 0.05, integ)) == 0, (order, k)
            assert stats[k]["samples"] == W * H * SPP and stats[k]["work_units"] > 0


# ---- scene kinds, one case each, box jitter
def _scene_case(name, tmp):
    if name == "cornell_blob":
        return load_scene(name)
    s = pt.Scene()
    ls.add_random_spheres(s, 100, 8, 6, sphere0_emissive=True)       # no triangle at all: 8 spheres, 6 of them lights
    s.build_bvh()
    return s


@pytest.mark.parametrize("name", ["cornell_blob", "spheres", "far_pose"])
def test_scene_kinds(tmp_path, name):
    s = _scene_case("cornell_blob" if name == "far_pose" else name, str(tmp_path))
    o = oracle.OracleScene(s.arrays())
    flags = KINDS["box"]
    if name == "far_pose":            # beyond 64 scene extents (cornell_blob's extent is 2): the tile kernel's fallback
        pos, dist, focal, view = view_ref.far_pose(200.0)
        cases = [(1, 0.0)]            # (the pose sees the outside of the walls, black to integrator 0)
    else:
        pos, dist, focal, view = POS, 1.0, 3.0, VIEWS["generic"]
        cases = [(0, 0.0), (1, 0.05)]
    with pt.Renderer(s, 0) as r:
        for integrator, radius in cases:
            cam = _cam(radius, pos=pos, dist=dist, focal=focal)
            v = pt.make_view(view[0], view[1], view[2], view[3])
            img, st = r.render(cam, W, H, SPP, BOUNCES, integrator, SEED, flags, view=v)
            ref, cnt = jitter_ref.render(o, _rcam(radius, pos=pos, dist=dist, focal=focal), view, flags, SPP, BOUNCES, integrator,
                                         SEED, return_counters=True)
            assert _same(img, ref) == 0, (name, integrator, radius)
            assert st["samples"] == W * H * SPP and st["rays_reference"] == cnt["traces"]
            assert (st["work_units"] > 0) == (name != "far_pose")
            assert np.count_nonzero(np.asarray(ref).max(axis=2) > 0) > 0                   # (the shot sees light at all)


# ---- features: the ray through the footprint's centre
def _features_of(rays, tri, t):
    o, d = rays
    hit = tri >= 0
    pos = np.zeros((len(tri), 3), dtype=F)
    for k in range(3):
        step = d[:, k] * t
        pos[:, k] = o[:, k] + step
    pos[~hit] = 0
    return hit, pos


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_features(renderers, osc, view):
    r = renderers["default"]
    cam, rcam = _cam(0.05), _rcam(0.05)
    plain = r.features(cam, W, H, view=_view(view))
    for kind in sorted(KINDS):                                       # box and tent alike
        feat = r.features(cam, W, H, view=_view(view), flags=KINDS[kind])
        rays = jitter_ref.centre_rays(rcam, VIEWS[view], W, H)
        tri, t = oracle.trace_batch(osc, rays[0], rays[1])
        hit, pos = _features_of(rays, tri, t)
        prim = feat["prim"].reshape(-1)
        assert hit.sum() > W * H // 2
        assert np.array_equal(np.where(prim >= 0, prim & ~pt.PT_FEATURE_EMISSIVE, -1), tri)
        assert jitter_ref.same_bits(feat["depth"].reshape(-1), t) == 0
        assert jitter_ref.same_bits(feat["position"].reshape(-1, 3), pos) == 0
        assert feat.tobytes() != plain.tobytes()
    # without the flag: today's corner ray, whatever else the flags say
    corner = [jitter_ref.ray(rcam, VIEWS[view], x, y, 0.0, 0.0, False) for y in range(H) for x in range(W)]
    rays = (np.array([c[0] for c in corner], dtype=F), np.array([c[1] for c in corner], dtype=F))
    tri, t = oracle.trace_batch(osc, rays[0], rays[1])
    hit, pos = _features_of(rays, tri, t)
    assert jitter_ref.same_bits(plain["depth"].reshape(-1), t) == 0
    assert jitter_ref.same_bits(plain["position"].reshape(-1, 3), pos) == 0
    assert r.features(cam, W, H, view=_view(view), flags=NPC).tobytes() == plain.tobytes()


# ---- pt_cli
def _cli(*args):
    obj = os.path.join(MODELS, "cornell.obj")
    base = [CLI, "--obj", obj, "--quiet"]
    return subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_jitter(osc, tmp_path):
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    size = ["--width", W, "--height", H, "--bounces", BOUNCES, "--seed", SEED, "--radius", 0.05]
    r = _cli(*size, "--jitter", "tent", "--spp", SPP, "--pfm", t("a.pfm"), "--out", t("a.ppm"))
    assert r.returncode == 0, r.stderr
    assert _same(pt.read_pfm(t("a.pfm")), _ref(osc, "tent", "null", 0.05, 0)) == 0
    # the same through a session file, stopped half way: the flags travel in the file
    r = _cli(*size, "--jitter", "tent", "--spp", 2, "--session", t("s.ptses"), "--out", t("b1.ppm"))
    assert r.returncode == 0, r.stderr
    assert pt.session_file_info(t("s.ptses"))["params"].flags == KINDS["tent"]
    r = _cli("--resume-session", t("s.ptses"), "--spp", 2, "--pfm", t("b.pfm"), "--out", t("b.ppm"))
    assert r.returncode == 0, r.stderr
    assert open(t("b.pfm"), "rb").read() == open(t("a.pfm"), "rb").read()
    # the same kind on the command line is no conflict, the other one is
    r = _cli("--resume-session", t("s.ptses"), "--jitter", "tent", "--spp", 1, "--out", t("c.ppm"))
    assert r.returncode == 0, r.stderr
    r = _cli("--resume-session", t("s.ptses"), "--jitter", "box", "--spp", 1, "--out", t("c.ppm"))
    assert r.returncode == 2 and "--jitter contradicts the resumed file" in r.stderr
    r = _cli(*size, "--jitter", "gauss")
    assert r.returncode == 2 and "--jitter is box or tent" in r.stderr
    # --aov with --jitter: the feature rays go through the pixels' centres
    r = _cli(*size, "--jitter", "box", "--spp", 1, "--aov", t("j"), "--out", t("d.ppm"))
    assert r.returncode == 0, r.stderr
    r = _cli(*size, "--spp", 1, "--aov", t("p"), "--out", t("e.ppm"))
    assert r.returncode == 0, r.stderr
    assert open(t("j_depth.pfm"), "rb").read() != open(t("p_depth.pfm"), "rb").read()
