"""The oriented camera on the GPU (include/pt/pt.h, pt_view): every render path through a view equals view_ref -- the
oracle's per-pixel loop restated around the numpy restatement of the oriented ray -- in every bit.  Cornell box,
24 x 16, 3-4 samples, 3 bounces, seed 1234."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS, ROOT, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib
from cudapathtracer_amd import make_view                     # (the parent has no such name: every test here errors there)
import oracle
import view_ref

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ROOT, "cudapathtracer_amd", "pt_cli")
W, H, SPP, BOUNCES, SEED = 24, 16, 4, 3, 1234
POS = (0.0, 1.0, 3.0)          # the reference camera's position: in front of the box's open side
POS_IN = (0.6, 1.0, 0.3)       # inside the box: the yawed camera looks at the wall at -x
GENERIC = view_ref.generic(POS)
# (position, view) pairs the cases are drawn from
SHOTS = {
    "generic": (POS, GENERIC),
    "yaw90": (POS_IN, view_ref.YAW90),
    "generic_film": (POS, view_ref.with_film(GENERIC, (1.5, 1.0))),
}
# shot, lens radius
CASES = [("generic", 0.0), ("yaw90", 0.0), ("generic", 0.05), ("yaw90", 0.05), ("generic_film", 0.0), ("generic_film", 0.05)]


def _view(v):
    return make_view(v[0], v[1], v[2], v[3])


def _cam(pos, radius, w=W, h=H):
    return pt.make_camera(pos, 1.0, 3.0, radius, w, h), (tuple(pos), 1.0, 3.0, radius, w, h)


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


def _ref(osc, shot, radius, integrator, spp=SPP, w=W, h=H):
    pos, view = SHOTS[shot]
    rcam = (tuple(pos), 1.0, 3.0, radius, w, h)
    return view_ref.render_cached("cornell", osc, rcam, view, spp, BOUNCES, integrator, SEED)


def _same(img, ref64):
    return view_ref.same_bits(img, np.asarray(ref64).astype(F))


# ---- the plain render on all three kernel families
PATHS = {
    "wavefront_unidir": ("default", 0, 0),
    "wavefront_head": ("default", 1, 0),
    "tile_reference_walk_unidir": ("default", 0, pt.PT_FLAG_REFERENCE_TRAVERSAL),
    "tile_reference_walk_head": ("default", 1, pt.PT_FLAG_REFERENCE_TRAVERSAL),
    "tile_head_wf_off": ("tile_head", 1, 0),
}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("shot,radius", CASES)
def test_render_through_a_view(renderers, osc, shot, radius, path):
    which, integrator, flags = PATHS[path]
    pos, view = SHOTS[shot]
    cam, _ = _cam(pos, radius)
    img, st = renderers[which].render(cam, W, H, SPP, BOUNCES, integrator, SEED, flags, view=_view(view))
    ref = _ref(osc, shot, radius, integrator)
    assert st["samples"] == W * H * SPP
    assert (st["work_units"] > 0) == path.startswith("wavefront")      # the kernel family the case is about
    assert _same(img, ref) == 0, (shot, radius, path)
    assert np.count_nonzero(ref) > W * H                               # (the shot sees the scene)


# ---- integrator 0's wavefront kernels have instances of their own for a view: every one of them.  The Cornell box
# fits the LDS tree, so the default renderer runs the LDS-walk instances; PT_WF_LDS_TREE=0 gives the others.
INSTANCES = {
    "lds_walk": ({}, 0),
    "memory_walk": ({"PT_WF_LDS_TREE": "0"}, 0),
    "count_lds_walk": ({}, pt.PT_FLAG_COUNT),
    "count_memory_walk": ({"PT_WF_LDS_TREE": "0"}, pt.PT_FLAG_COUNT),
    "count_min_waves_4": ({"PT_WF_MIN_WAVES": "4"}, pt.PT_FLAG_COUNT),
    "min_waves_4": ({"PT_WF_MIN_WAVES": "4"}, 0),
    "min_waves_6": ({"PT_WF_MIN_WAVES": "6"}, 0),
}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_every_view_instance_of_the_unidir_wavefront_kernel(scene, osc, name):
    env, flags = INSTANCES[name]
    r = _renderer(scene, env)
    try:
        for radius in (0.0, 0.05):
            cam, _ = _cam(POS, radius)
            img, st = r.render(cam, W, H, SPP, BOUNCES, 0, SEED, flags, view=_view(GENERIC))
            assert st["work_units"] > 0 and _same(img, _ref(osc, "generic", radius, 0)) == 0, (name, radius)
            if flags & pt.PT_FLAG_COUNT:
                assert st["node_tests"] > 0
            if name in ("lds_walk", "memory_walk"):                # the accumulating twins
                with r.accumulator(cam, W, H, BOUNCES, 0, SEED, view=_view(GENERIC)) as acc:
                    acc.add(1)
                    acc.add(3)
                    assert _same(acc.image(), _ref(osc, "generic", radius, 0)) == 0, (name, radius)
    finally:
        r.close()


def test_a_view_is_not_ignored(renderers):
    """A yawed view's image differs from the NULL view's: a view that is silently dropped cannot pass."""
    r = renderers["default"]
    cam, _ = _cam(POS_IN, 0.0)
    for integrator, flags in ((0, 0), (1, 0), (0, pt.PT_FLAG_REFERENCE_TRAVERSAL)):
        null, _ = r.render(cam, W, H, SPP, BOUNCES, integrator, SEED, flags)
        yaw, _ = r.render(cam, W, H, SPP, BOUNCES, integrator, SEED, flags, view=_view(view_ref.YAW90))
        assert view_ref.same_bits(null, yaw) > W * H


def test_an_invalid_view_is_refused(renderers):
    r = renderers["default"]
    cam, _ = _cam(POS, 0.0)
    bad = make_view((1.01, 0, 0), (0, 1, 0), (0, 0, 1))
    for call in (lambda: r.render(cam, W, H, 1, view=bad), lambda: r.accumulator(cam, W, H, view=bad),
                 lambda: r.features(cam, W, H, view=bad)):
        with pytest.raises(pt.PtError) as e:
            call()
        assert e.value.code == pt.PT_E_INVALID and "orthonormal" in str(e.value)


# ---- split units: every chunk of a pixel gets the same set-up direction
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_split_units(renderers, osc, radius, integrator):
    pos, view = SHOTS["generic"]
    cam, _ = _cam(pos, radius)
    img, st = renderers["chunks"].render(cam, W, H, SPP, BOUNCES, integrator, SEED, view=_view(view))
    assert st["split_pixels"] > 0
    assert _same(img, _ref(osc, "generic", radius, integrator)) == 0


# ---- shards and pixel orders
def _shard_pixels(w, h, index, count, tile):
    n = C.c_uint32(0)
    _lib.check(_lib.lib().pt_shard_pixels(w, h, index, count, tile, tile, None, 0, C.byref(n)))
    pix = np.zeros(max(n.value, 1), dtype=np.uint32)
    _lib.check(_lib.lib().pt_shard_pixels(w, h, index, count, tile, tile, pix.ctypes.data, len(pix), C.byref(n)))
    return pix[:n.value]


@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_shards(renderers, osc, radius):
    r = renderers["default"]
    pos, view = SHOTS["generic"]
    cam, _ = _cam(pos, radius)
    ref = np.asarray(_ref(osc, "generic", radius, 0)).astype(F)
    img, st = r.render(cam, W, H, SPP, BOUNCES, 0, SEED, shard_index=1, shard_count=2, view=_view(view))
    mine = _shard_pixels(W, H, 1, 2, 0)
    assert 0 < len(mine) < W * H and st["samples"] == len(mine) * SPP
    want = np.zeros_like(ref)
    want.reshape(-1, 3)[mine] = ref.reshape(-1, 3)[mine]
    assert view_ref.same_bits(img, want) == 0
    # a shard that owns no pixel: nothing is launched, the image stays zero
    img, st = r.render(cam, W, H, SPP, BOUNCES, 0, SEED, shard_index=7, shard_count=8, tile_w=256, tile_h=256, view=_view(view))
    assert st["samples"] == 0 and not img.any()


def test_morton_order(renderers, osc):
    n = 16
    pos, view = SHOTS["generic"]
    cam, rcam = _cam(pos, 0.0, n, n)
    ref = view_ref.render_cached("cornell", osc, rcam, view, 3, BOUNCES, 0, SEED).astype(F)
    img, _ = renderers["default"].render(cam, n, n, 3, BOUNCES, 0, SEED, pixel_order=pt.PT_ORDER_MORTON, view=_view(view))
    want = np.zeros((n * n, 3), dtype=F)
    for y in range(n):
        for x in range(n):
            want[view_ref.morton(x, y)] = ref[y, x]
    assert view_ref.same_bits(img, want) == 0


# ---- the accumulator keeps its view
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_accumulator(renderers, osc, radius, integrator):
    r = renderers["default"]
    pos, view = SHOTS["generic"]
    cam, rcam = _cam(pos, radius)
    v = _view(view)
    with r.accumulator(cam, W, H, BOUNCES, integrator, SEED, view=v) as acc:
        got = acc.view
        assert got is not None and bytes(got) == bytes(v)
        acc.add(2)
        acc.add(2)
        assert _same(acc.image(), _ref(osc, "generic", radius, integrator)) == 0
        # freeze half of the pixels (not pixel 0, the reference's quirk lens pixel): the adaptive pass
        # (init_active_states) samples the rest
        mask = np.zeros((H, W), dtype=np.uint8)
        mask[::2, 1::2] = 1
        mask[1::2, ::2] = 1
        acc.freeze(mask)
        acc.add(2)
        counts = acc.counts()
        assert np.array_equal(counts, np.where(mask != 0, 4, 6))
        ref = view_ref.render(osc, rcam, view, 0, BOUNCES, integrator, SEED, counts=counts)
        assert view_ref.same_bits(acc.mean64(), ref) == 0
    with r.accumulator(cam, W, H, BOUNCES, integrator, SEED) as acc:
        assert acc.view is None


# ---- features: the oriented pinhole ray, whatever the lens
@pytest.mark.parametrize("shot,radius", [("generic", 0.0), ("yaw90", 0.05), ("generic_film", 0.0)])
def test_features(renderers, shot, radius):
    r = renderers["default"]
    pos, view = SHOTS[shot]
    cam, rcam = _cam(pos, radius)
    feat = r.features(cam, W, H, view=_view(view))
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = view_ref.rays(rcam, view, xs.reshape(-1), ys.reshape(-1), False)
    tri, t = r.trace(o, d)
    prim = feat["prim"].reshape(-1)
    hit = prim >= 0
    assert hit.sum() > W * H // 2
    assert np.array_equal(np.where(hit, prim & ~pt.PT_FEATURE_EMISSIVE, -1), tri)
    assert view_ref.same_bits(feat["depth"].reshape(-1), t) == 0
    want = np.zeros((W * H, 3), dtype=F)
    for k in range(3):
        step = d[:, k] * t
        want[:, k] = o[:, k] + step
    want[~hit] = 0
    assert view_ref.same_bits(feat["position"].reshape(-1, 3), want) == 0


# ---- session files: format version 3 carries the view
def test_session_file(renderers, tmp_path):
    r = renderers["default"]
    pos, view = SHOTS["generic_film"]
    cam, _ = _cam(pos, 0.05)
    v = _view(view)
    f, f2 = str(tmp_path / "s.ptses"), str(tmp_path / "plain.ptses")

    def steps(acc, est, out):
        for _ in range(2):
            acc.add(2)
            out.append(est.update(tol=0.2))
        out.append(est.freeze(tol=0.2))
        acc.add(2)
        out.append(est.update(tol=0.2))

    # the uninterrupted run
    a_log = []
    with r.accumulator(cam, W, H, BOUNCES, 0, SEED, view=v) as acc:
        est = acc.noise()
        acc.add(2)
        a_log.append(est.update(tol=0.2))
        steps(acc, est, a_log)
        a_img, a_cnt, a_state = acc.mean64(), acc.counts(), est.read()
    # the same, saved mid-run (between a pass and its update), destroyed, loaded and continued
    b_log = []
    with r.accumulator(cam, W, H, BOUNCES, 0, SEED, view=v) as acc:
        est = acc.noise()
        acc.add(2)
        acc.save_session(f, noise=est)
        with pytest.raises(pt.PtError) as e:                       # format 1 has no room for a view
            acc.save(str(tmp_path / "c.ptacc"))
        assert e.value.code == pt.PT_E_INVALID and "pt_session_save" in str(e.value) and "view" in str(e.value)
    blob = open(f, "rb").read()
    assert blob[8:16] == np.array([3, 256], dtype="<u4").tobytes()
    assert blob[192:236] == bytes(v) and blob[236:256] == bytes(20)
    assert len(blob) == 256 + W * H * (48 + 40)
    got = pt.session_file_view(f)
    assert got is not None and bytes(got) == bytes(v)
    acc, est = r.load_session(f)
    with acc:
        assert bytes(acc.view) == bytes(v) and acc.samples == 2
        b_log.append(est.update(tol=0.2))
        steps(acc, est, b_log)
        assert b_log == a_log
        assert view_ref.same_bits(acc.mean64(), a_img) == 0 and np.array_equal(acc.counts(), a_cnt)
        for x, y in zip(est.read(), a_state):
            assert view_ref.same_bits(x, y) == 0
    # without a view the file is version 2, as it always was
    with r.accumulator(cam, W, H, BOUNCES, 0, SEED) as acc:
        acc.add(1)
        acc.save_session(f2)
    blob = open(f2, "rb").read()
    assert blob[8:16] == np.array([2, 192], dtype="<u4").tobytes() and len(blob) == 192 + W * H * 48
    assert pt.session_file_view(f2) is None


def test_one_rank_group(renderers, osc):
    r = renderers["default"]
    pos, view = SHOTS["generic"]
    cam, _ = _cam(pos, 0.05)
    with pt.Group([r]) as g:
        img, st = g.render(cam, W, H, SPP, BOUNCES, 0, SEED, view=_view(view))
    one, _ = r.render(cam, W, H, SPP, BOUNCES, 0, SEED, view=_view(view))
    assert view_ref.same_bits(img, one) == 0 and _same(img, _ref(osc, "generic", 0.05, 0)) == 0
    assert st["samples"] == W * H * SPP


# ---- pt_cli
def _cli(*args):
    obj = os.path.join(MODELS, "cornell.obj")
    base = [CLI, "--obj", obj, "--quiet"]
    return subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_look_at(renderers, tmp_path):
    t = lambda name: str(tmp_path / name)                                      # noqa: E731
    target, up, vfov = (0.3, 0.7, -0.2), (0.1, 1.0, 0.05), 40.0
    size = ["--width", W, "--height", H, "--bounces", BOUNCES, "--seed", SEED]
    shot = ["--look-at", "%r,%r,%r" % target, "--up", "%r,%r,%r" % up, "--vfov", vfov, "--radius", 0.05]
    cam, _ = _cam(POS, 0.05)
    v = pt.look_at(POS, target, up, vfov=vfov, cam=cam)
    api, _ = renderers["default"].render(cam, W, H, SPP, BOUNCES, 0, SEED, view=v)
    r = _cli(*size, *shot, "--spp", SPP, "--pfm", t("a.pfm"), "--out", t("a.ppm"))
    assert r.returncode == 0, r.stderr
    assert view_ref.same_bits(pt.read_pfm(t("a.pfm")), api) == 0
    # the same through a session file, stopped half way: the view travels in the file
    r = _cli(*size, *shot, "--spp", 2, "--session", t("s.ptses"), "--out", t("b1.ppm"))
    assert r.returncode == 0, r.stderr
    assert bytes(pt.session_file_view(t("s.ptses"))) == bytes(v)
    r = _cli("--resume-session", t("s.ptses"), "--spp", 2, "--pfm", t("b.pfm"), "--out", t("b.ppm"))
    assert r.returncode == 0, r.stderr
    assert open(t("b.pfm"), "rb").read() == open(t("a.pfm"), "rb").read()
    # the same view on the command line is no conflict, another one is; a checkpoint cannot hold a view
    r = _cli("--resume-session", t("s.ptses"), *shot[:6], "--spp", 1, "--out", t("c.ppm"))
    assert r.returncode == 0, r.stderr
    r = _cli("--resume-session", t("s.ptses"), "--look-at", "0,1,0", "--spp", 1, "--out", t("c.ppm"))
    assert r.returncode == 2 and "contradict the resumed file" in r.stderr
    r = _cli(*size, *shot, "--spp", 1, "--checkpoint", t("c.ptacc"), "--out", t("c.ppm"))
    assert r.returncode == 1 and "pt_accum_save" in r.stderr and "pt_session_save" in r.stderr
