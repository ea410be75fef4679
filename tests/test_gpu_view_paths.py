"""The oriented camera (include/pt/pt.h, pt_view) on every kernel instance, scene kind, pose and consumer that
tests/test_gpu_view.py leaves out: all eight render_tiles_view instances, integrator 1's wavefront kernels in their
counting and 4-wave builds, scenes with spheres, long light lists and a tree too large for LDS, mirrored, rolled,
axis-aligned, blind, barely valid, very wide and very narrow views, oriented cameras beyond the fast walk's 64 scene
extents, and the entry points that carry a view of their own.  Every image equals view_ref -- the oracle's per-pixel
loop around the numpy restatement of the oriented ray -- in every bit.  24 x 16, 3 samples, 3 bounces, seed 1234
unless a case says otherwise.  tests/test_view_shots_host.py shows on the CPU that the shots discriminate."""
import os

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import make_view, shard
import light_scenes as ls
import oracle
import view_ref

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCES, SEED = 24, 16, 3, 3, 1234
POS = (0.0, 1.0, 3.0)          # the reference camera's position: in front of the box's open side
POS_IN = (0.6, 1.0, 0.3)       # inside the box
RT, RB, CNT = pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH, pt.PT_FLAG_COUNT
FAR_M = [100.0, 128.0, float(np.nextafter(F(128), F(np.inf))), 200.0, 2e4]   # cornell_blob's extent is 2: the bound is 128


def _look(pos, target):
    r, u, b = view_ref.look_at64(pos, target, (0.1, 1.0, 0.05))
    return (tuple(float(v) for v in r), tuple(float(v) for v in u), tuple(float(v) for v in b), (1, 1))


# name: (pos, dist_from_film, focal_length, view)
SHOTS = dict(view_ref.SHOTS_EXTRA)
SHOTS["generic"] = (POS, 1.0, 3.0, view_ref.generic(POS))
SHOTS["yaw90"] = (POS_IN, 1.0, 3.0, view_ref.YAW90)
SHOTS["standin_inside"] = ((0.0, 2.6, 4.0), 1.0, 3.0, _look((0.0, 2.6, 4.0), (3.0, 2.0, -2.0)))   # between its walls
for _m in FAR_M:
    SHOTS["far_%.9g" % _m] = view_ref.far_pose(_m)


def _far(m):
    return "far_%.9g" % m


def _view(shot):
    v = SHOTS[shot][3]
    return make_view(v[0], v[1], v[2], v[3])


def _cam(shot, radius, w=W, h=H):
    pos, dist, focal, _ = SHOTS[shot]
    return pt.make_camera(pos, dist, focal, radius, w, h)


def _rcam(shot, radius, w=W, h=H):
    pos, dist, focal, _ = SHOTS[shot]
    return (tuple(pos), dist, focal, radius, w, h)


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


class Stage:
    """One scene: its arrays, its oracle scene, one renderer per environment and the references, each made once."""

    def __init__(self, name, scene):
        self.name, self.scene = name, scene
        self.arrays = scene.arrays()
        self.osc = oracle.OracleScene(self.arrays)
        self._renderers = {}

    def renderer(self, env=None):
        key = tuple(sorted((env or {}).items()))
        if key not in self._renderers:
            self._renderers[key] = _renderer(self.scene, dict(key))
        return self._renderers[key]

    def ref(self, shot, radius, integrator, w=W, h=H, spp=SPP):
        """(f64 image, the oracle's counters) of the shot, shared: read-only."""
        return view_ref.render_cached(self.name, self.osc, _rcam(shot, radius, w, h), SHOTS[shot][3], spp, BOUNCES, integrator,
                                      SEED, return_counters=True)

    def close(self):
        for r in self._renderers.values():
            r.close()
        self._renderers = {}


def _build(name, dirpath, request):
    if name == "standin":
        return request.getfixturevalue("standin_scene")
    if name in ("cornell", "cornell_blob", "quirks"):
        return load_scene(name)
    s = pt.Scene()
    if name == "spheres":                                   # no triangle at all: 8 spheres, 6 of them lights
        ls.add_random_spheres(s, 100, 8, 6, sphere0_emissive=True)
    elif name == "mixed":                                   # a soup with 3 emissive triangles and 6 spheres, 3 emissive
        s.load_obj(ls.write_lit_soup(dirpath, 100, 3), mtl_basepath=dirpath + "/")
        ls.add_random_spheres(s, 100, 6, 3)
    else:
        raise KeyError(name)
    s.build_bvh()
    return s


@pytest.fixture(scope="module")
def stages(request, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Stage(name, _build(name, str(tmp_path_factory.mktemp("view_" + name)), request))
        return made[name]

    yield get
    for s in made.values():
        s.close()


def _same(img, ref64):
    return view_ref.same_bits(img, np.asarray(ref64).astype(F))


def _check(stage, img, st, shot, radius, integrator, w=W, h=H, spp=SPP, what=None):
    ref, cnt = stage.ref(shot, radius, integrator, w, h, spp)
    print("%s %s r=%g i=%d %s: differing %d, samples %d, rays_reference %d (oracle %d), rays_traced %d, work_units %d"
          % (stage.name, shot, radius, integrator, what, _same(img, ref), st["samples"], st["rays_reference"], cnt["traces"],
             st["rays_traced"], st["work_units"]))
    assert _same(img, ref) == 0, (stage.name, shot, radius, integrator, what)
    assert st["samples"] == w * h * spp
    assert st["rays_reference"] == cnt["traces"]
    return ref, cnt


# ---------------------------------------------------------------- a. every render_tiles_view<I, R, C> instance
def _tile_instances():
    """name: (environment, integrator, flags, fast-walk tile kernel expected)."""
    base = {
        "i0_refwalk": ({}, 0, RT),                                        # <0, true, *>
        "i0_reference_bvh": ({}, 0, RB),                                  # <0, false, *>
        "i1_refwalk": ({}, 1, RT),                                        # <1, true, *>
        "i1_head_wf_off": ({"PT_HEAD_WF": "0"}, 1, 0),                    # <1, false, *>, the BVH4 walk
        "i1_reference_bvh": ({}, 1, RB),                                  # <1, false, *>, the culled reference walk
        "i0_reference_bvh_fast4_off": ({"PT_TILE_FAST4": "0"}, 0, RB),
        "i1_head_wf_off_fast4_off": ({"PT_HEAD_WF": "0", "PT_TILE_FAST4": "0"}, 1, 0),
        "i1_reference_bvh_fast4_off": ({"PT_TILE_FAST4": "0"}, 1, RB),
    }
    out = {}
    for k, (env, integ, flags) in base.items():
        out[k] = (env, integ, flags)
        out[k + "_count"] = (env, integ, flags | CNT)
    return out


TILE_INSTANCES = _tile_instances()


@pytest.mark.parametrize("name", sorted(TILE_INSTANCES))
def test_every_tile_kernel_instance(stages, name):
    env, integ, flags = TILE_INSTANCES[name]
    st_ = stages("cornell")
    r = st_.renderer(env)
    for radius in (0.0, 0.05):
        img, st = r.render(_cam("generic", radius), W, H, SPP, BOUNCES, integ, SEED, flags, view=_view("generic"))
        _check(st_, img, st, "generic", radius, integ, what=name)
        assert st["work_units"] == 0                                      # the tile kernel
        if flags & CNT:
            assert st["node_tests"] > 0 and st["tri_tests"] > 0


@pytest.mark.parametrize("integ", [0, 1])
def test_per_triangle_counts_match_reference_through_a_view(stages, integ):
    """The oriented twin of test_gpu_parity.py's test_per_triangle_counts_match_reference: with the reference
    traversal and both shortcuts off the render performs exactly the reference's trace() calls."""
    st_ = stages("cornell")
    r = st_.renderer()
    flags = RT | pt.PT_FLAG_NO_PRIMARY_CACHE | pt.PT_FLAG_NO_DEAD_PATH_SKIP | CNT | pt.PT_FLAG_TRI_COUNTS
    for radius in (0.0, 0.05):
        want = np.zeros(len(st_.osc.tris), dtype=np.uint32)
        ref, cnt = view_ref.render(st_.osc, _rcam("generic", radius), SHOTS["generic"][3], SPP, BOUNCES, integ, SEED,
                                   tri_counts=want, return_counters=True)
        img, st = r.render(_cam("generic", radius), W, H, SPP, BOUNCES, integ, SEED, flags, view=_view("generic"))
        counts = r.tri_counts()
        assert _same(img, ref) == 0
        assert np.array_equal(counts, want)
        assert int(counts.sum()) == st["tri_tests"] == cnt["tri_tests"]
        assert st["rays_traced"] == st["rays_reference"] == cnt["traces"]
        # the fast path's own counts: the same image with strictly fewer triangle tests
        img2, st2 = r.render(_cam("generic", radius), W, H, SPP, BOUNCES, integ, SEED, CNT | pt.PT_FLAG_TRI_COUNTS,
                             view=_view("generic"))
        fast = r.tri_counts()
        assert _same(img2, ref) == 0
        assert 0 < int(fast.sum()) < int(counts.sum())
        assert 0 < st2["tri_tests"] < st["tri_tests"]


# ---------------------------------------------------------------- b. integrator 1's wavefront kernels
HEAD_INSTANCES = {
    "count": ({}, CNT),                                                       # render_head_wf<true, 5>
    "count_lds_tree_off": ({"PT_WF_LDS_TREE": "0"}, CNT),
    "min_waves_4": ({"PT_HEAD_MIN_WAVES": "4"}, 0),                           # render_head_wf<false, 4>
    "min_waves_4_lds_tree_off": ({"PT_HEAD_MIN_WAVES": "4", "PT_WF_LDS_TREE": "0"}, 0),
    "lds_tree_off": ({"PT_WF_LDS_TREE": "0"}, 0),                             # render_head_wf<false, 5>, records by memory
}


@pytest.mark.parametrize("name", sorted(HEAD_INSTANCES))
def test_every_head_wavefront_instance(stages, name):
    """The view is taken under a.oriented in the lens stage: a lens camera."""
    env, flags = HEAD_INSTANCES[name]
    st_ = stages("cornell")
    r = st_.renderer(env)
    for shot in ("generic", "yaw90"):
        img, st = r.render(_cam(shot, 0.05), W, H, SPP, BOUNCES, 1, SEED, flags, view=_view(shot))
        _check(st_, img, st, shot, 0.05, 1, what=name)
        assert st["work_units"] > 0
        if flags & CNT:
            assert st["node_tests"] > 0 and st["tri_tests"] > 0


# ---------------------------------------------------------------- c. scenes
def _features_ref(arrays, rcam, view, trace):
    """The (H, W) FEATURE array of pt_render_features through a view, composed on the host (denoise_ref.features_ref
    with the oriented pinhole ray): view_ref.rays, `trace(origins, directions) -> (prim, t)`, then the scene arrays."""
    w, h = rcam[4], rcam[5]
    ys, xs = np.mgrid[0:h, 0:w]
    o, d = view_ref.rays(rcam, view, xs.reshape(-1), ys.reshape(-1), False)
    prim, t = trace(o, d)
    prim = np.asarray(prim, dtype=np.int32)
    t = np.asarray(t, dtype=F)
    tris, mats, sph = arrays["tris"], arrays["mats"], arrays["spheres"]
    nt = len(tris)
    f = np.zeros(w * h, dtype=pt.FEATURE)
    f["prim"] = -1
    f["depth"] = t
    for q in np.nonzero(prim >= 0)[0]:
        k = int(prim[q])
        step = (d[q] * t[q]).astype(F)
        pos = (o[q] + step).astype(F)
        if k < nt:
            m = mats[tris[k]["mat"]]
            alb, emi = m["albedo"], m["emission"]
            nrm = np.array([tris[k]["nx"], tris[k]["ny"], tris[k]["nz"]], dtype=F)
        else:
            s = sph[k - nt]
            alb, emi = s["diffuse"], s["emission"]
            nrm = ((pos - s["pos"].astype(F)).astype(F) / F(s["rad"])).astype(F)
        f[q]["albedo"] = alb.astype(F)
        f[q]["normal"] = nrm
        f[q]["position"] = pos
        f[q]["prim"] = k | (pt.PT_FEATURE_EMISSIVE if emi[0] != 0 else 0)
    return f.reshape(h, w)


def _feature_diffs(got, ref):
    """{field: records that differ in any bit}, the non-zero entries only."""
    out = {}
    for k in ("prim", "depth", "position", "normal", "albedo", "reserved"):
        a = np.ascontiguousarray(got[k]).view(np.uint32).reshape(got.size, -1)
        b = np.ascontiguousarray(ref[k]).view(np.uint32).reshape(ref.size, -1)
        n = int(np.count_nonzero((a != b).any(axis=1)))
        if n:
            out[k] = n
    return out


SCENE_CASES = [(s, shot, w, h, spp) for s in ("cornell_blob", "quirks", "spheres", "mixed") for shot in ("generic", "down")
               for w, h, spp in [(W, H, SPP)]] + [("standin", "standin_inside", 16, 8, 2)]
SCENE_PATHS = {"wavefront_unidir": (0, 0), "wavefront_head": (1, 0), "tile_reference_walk_unidir": (0, RT)}


@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("scene,shot,w,h,spp", SCENE_CASES, ids=["%s-%s" % c[:2] for c in SCENE_CASES])
def test_scene_kinds(stages, scene, shot, w, h, spp, radius):
    st_ = stages(scene)
    r = st_.renderer()
    if scene == "spheres":
        assert len(st_.arrays["tris"]) == 0 and len(st_.arrays["spheres"]) == 8 and len(st_.arrays["lights"]) == 6
    if scene == "mixed":
        assert len(st_.arrays["spheres"]) == 6 and len(st_.arrays["lights"]) == 3 + 3
    for path, (integ, flags) in sorted(SCENE_PATHS.items()):
        img, st = r.render(_cam(shot, radius, w, h), w, h, spp, BOUNCES, integ, SEED, flags, view=_view(shot))
        ref, _ = _check(st_, img, st, shot, radius, integ, w, h, spp, what=path)
        assert (st["work_units"] > 0) == path.startswith("wavefront")
        assert np.count_nonzero(ref) > 0 and np.isfinite(img).all()            # (the shot sees lit surfaces)


@pytest.mark.parametrize("scene,shot,w,h,spp", SCENE_CASES, ids=["%s-%s" % c[:2] for c in SCENE_CASES])
def test_scene_kinds_features(stages, scene, shot, w, h, spp):
    """prim, depth and position against Renderer.trace of the restatement's rays (and with them albedo, and the
    normal: of a sphere hit (position - pos) / rad in float32), whatever the lens."""
    st_ = stages(scene)
    r = st_.renderer()
    nt = len(st_.arrays["tris"])
    for radius in (0.0, 0.05):
        got = r.features(_cam(shot, radius, w, h), w, h, view=_view(shot))
        ref = _features_ref(st_.arrays, _rcam(shot, radius, w, h), SHOTS[shot][3], r.trace)
        assert not _feature_diffs(got, ref), (scene, shot, radius, _feature_diffs(got, ref))
        assert got.tobytes() == ref.tobytes()
        hit = ref["prim"] >= 0
        assert hit.sum() > 0
        on_sphere = hit & ((ref["prim"] & ~pt.PT_FEATURE_EMISSIVE) >= nt)
        if scene == "spheres":
            assert on_sphere.sum() > 0 and (on_sphere == hit).all()
            sp = st_.arrays["spheres"][(ref["prim"][on_sphere] & ~pt.PT_FEATURE_EMISSIVE) - nt]
            want = ((got["position"][on_sphere] - sp["pos"].astype(F)).astype(F) / sp["rad"].astype(F)[:, None]).astype(F)
            assert view_ref.same_bits(got["normal"][on_sphere], want) == 0
    # ... and the oracle's trace agrees with the device's on these rays
    cpu = _features_ref(st_.arrays, _rcam(shot, 0.0, w, h), SHOTS[shot][3], lambda o, d: oracle.trace_batch(st_.osc, o, d))
    assert not _feature_diffs(got, cpu), (scene, shot, _feature_diffs(got, cpu))


def test_standin_takes_the_memory_walk(stages):
    """The stand-in's tree does not fit in LDS: the counting render walks nodes from memory."""
    st_ = stages("standin")
    w, h, spp = 16, 8, 2
    for integ in (0, 1):
        img, st = st_.renderer().render(_cam("standin_inside", 0.05, w, h), w, h, spp, BOUNCES, integ, SEED, CNT,
                                        view=_view("standin_inside"))
        _check(st_, img, st, "standin_inside", 0.05, integ, w, h, spp, what="count")
        print("standin count i=%d: node_tests %d lds_node_tests %d spill_entries %d"
              % (integ, st["node_tests"], st["lds_node_tests"], st["spill_entries"]))
        assert st["work_units"] > 0
        assert st["spill_entries"] > 0 or st["node_tests"] - st["lds_node_tests"] > 0


# ---------------------------------------------------------------- d. poses
POSE_PATHS = {"wavefront_unidir": (0, 0), "wavefront_head": (1, 0), "tile_reference_walk_unidir": (0, RT)}


@pytest.mark.parametrize("radius", [0.0, 0.05])
@pytest.mark.parametrize("shot", sorted(view_ref.SHOTS_EXTRA))
def test_poses(stages, shot, radius):
    st_ = stages("cornell")
    r = st_.renderer()
    for path, (integ, flags) in sorted(POSE_PATHS.items()):
        img, st = r.render(_cam(shot, radius), W, H, SPP, BOUNCES, integ, SEED, flags, view=_view(shot))
        ref, cnt = _check(st_, img, st, shot, radius, integ, what=path)
        assert (st["work_units"] > 0) == path.startswith("wavefront")
        if shot == "away":
            # Every camera ray misses.  The reference integrators go on tracing a path whose weight the miss has zeroed
            # (rays_reference is the oracle's count, as everywhere); integrator 0 on the device traces nothing after it,
            # and its image is all zero bits.  Integrator 1 shades a camera miss as triangle 0 at t = 0 (the reference's
            # miss convention, kernel.cu:279-283), so its image is the reference's and not black.
            assert 0 < st["rays_traced"] <= st["rays_reference"]
            if integ == 0:
                assert not img.any() and not np.asarray(ref).any()
                assert st["rays_traced"] <= W * H * SPP < st["rays_reference"]
        else:
            assert np.count_nonzero(ref) > W * H
    if shot == "away":
        feat = r.features(_cam(shot, radius), W, H, view=_view(shot))
        none = np.zeros(1, dtype=pt.FEATURE)
        none["prim"], none["depth"] = -1, 1e5
        assert (feat["prim"] == -1).all() and (feat["depth"] == F(1e5)).all()
        assert feat.tobytes() == none.tobytes() * (W * H)


# ---------------------------------------------------------------- e. far oriented cameras
@pytest.mark.parametrize("flags", [0, RB], ids=["default", "reference_bvh"])
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("m", FAR_M, ids=lambda m: "%.9g" % m)
def test_far_oriented_camera(stages, m, integ, flags):
    st_ = stages("cornell_blob")
    shot = _far(m)
    img, st = st_.renderer().render(_cam(shot, 0.0), W, H, SPP, BOUNCES, integ, SEED, flags, view=_view(shot))
    ref, _ = _check(st_, img, st, shot, 0.0, integ, what="flags %d" % flags)
    # (the pose sees mostly the outside of the walls, black to integrator 0: tests/test_view_shots_host.py)
    lit = int(np.count_nonzero(np.asarray(ref).max(axis=2) > 0))
    assert lit > (W * H // 4 if integ == 1 else 0)
    assert (st["work_units"] > 0) == (m <= 128.0 and flags == 0)


@pytest.mark.parametrize("m", FAR_M, ids=lambda m: "%.9g" % m)
def test_far_oriented_camera_features(stages, m):
    """primary_features_view on both sides of ray_regular: the whole record against the host composition over the
    oracle's trace (as test_gpu_ray_ranges.py's test_far_camera_features)."""
    st_ = stages("cornell_blob")
    shot = _far(m)
    w, h = 37, 19
    ref = _features_ref(st_.arrays, _rcam(shot, 0.0, w, h), SHOTS[shot][3], lambda o, d: oracle.trace_batch(st_.osc, o, d))
    assert np.count_nonzero(ref["prim"] >= 0) > w * h // 4
    got = st_.renderer().features(_cam(shot, 0.0, w, h), w, h, view=_view(shot))
    assert not _feature_diffs(got, ref), (m, _feature_diffs(got, ref))
    assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("integ", [0, 1])
def test_far_lens_camera_straddles_the_bound(stages, integ):
    """A lens camera at exactly 64 extents whose basis tilts the lens disc along x: near_camera() passes it on its
    position, and the wavefront kernel starts rays on both sides of |x| = 128 (tests/test_view_shots_host.py)."""
    st_ = stages("cornell_blob")
    r = st_.renderer()
    shot = _far(128.0)
    cam, v = _cam(shot, 0.05), _view(shot)
    img, st = r.render(cam, W, H, SPP, BOUNCES, integ, SEED, view=v)
    assert st["work_units"] > 0
    ref, _ = _check(st_, img, st, shot, 0.05, integ, what="straddle")
    assert np.count_nonzero(ref) > 0
    with r.accumulator(cam, W, H, BOUNCES, integ, SEED, view=v) as acc:
        acc.add(1)
        acc.add(2)
        assert _same(acc.image(), ref) == 0


# ---------------------------------------------------------------- f. consumers
CONSUMER_SHOTS = ["generic", "yaw90"]


def _mine(w, h, index, count, tw=0, th=0):
    mask = np.zeros(w * h, dtype=bool)
    mask[shard.shard_pixels(w, h, index, count, tw or 8, th or 8)] = True
    return mask.reshape(h, w)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("shot", CONSUMER_SHOTS)
def test_render_device(stages, shot, integ):
    import torch
    st_ = stages("cornell")
    r = st_.renderer()
    ref32 = np.asarray(st_.ref(shot, 0.05, integ)[0]).astype(F)
    sentinel = F(-7.5)
    for index, count in ((0, 1), (1, 2)):
        buf = torch.full((H, W, 3), float(sentinel), dtype=torch.float32, device="cuda")
        st = r.render_device(_cam(shot, 0.05), buf.data_ptr(), W, H, SPP, BOUNCES, integ, SEED, shard_index=index,
                             shard_count=count, view=_view(shot))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        mine = _mine(W, H, index, count)
        assert 0 < mine.sum() and (mine.all() == (count == 1)) and st["samples"] == int(mine.sum()) * SPP
        assert view_ref.same_bits(got[mine], ref32[mine]) == 0
        assert (got[~mine] == sentinel).all()                                   # only the shard's pixels change


@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
def test_async_renders_with_different_views(stages, two_streams):
    """Two renders in flight, each with a view of its own (and the second with the other integrator): each frame
    equals its own reference.  Repeated, so that both flight slots are reused with the other view."""
    import torch
    st_ = stages("cornell")
    r = st_.renderer()
    cases = [("generic", 0), ("yaw90", 1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two_streams else [torch.cuda.Stream()] * 2
    bufs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    for rep in range(2):
        order = cases if rep == 0 else cases[::-1]
        for k, (shot, integ) in enumerate(order):
            s = streams[k]
            with torch.cuda.stream(s):
                bufs[k].zero_()
                r.render_device_async(_cam(shot, 0.05), bufs[k].data_ptr(), W, H, SPP, BOUNCES, integ, SEED,
                                      stream_ptr=s.cuda_stream, view=_view(shot))
        stats = [r.wait(), r.wait()]
        torch.cuda.synchronize()
        for k, (shot, integ) in enumerate(order):
            _check(st_, bufs[k].cpu().numpy(), stats[k], shot, 0.05, integ, what="async rep %d slot %d" % (rep, k))
            assert stats[k]["work_units"] > 0


@pytest.mark.parametrize("shot", CONSUMER_SHOTS)
def test_shards_sum_to_the_frame(stages, shot):
    st_ = stages("cornell")
    r = st_.renderer()
    w, h, n, tw, th = 37, 19, 3, 16, 8
    for integ in (0, 1):
        ref32 = np.asarray(st_.ref(shot, 0.05, integ, w, h)[0]).astype(F)
        total = np.zeros_like(ref32)
        seen = np.zeros((h, w), dtype=int)
        for k in range(n):
            part, st = r.render(_cam(shot, 0.05, w, h), w, h, SPP, BOUNCES, integ, SEED, shard_index=k, shard_count=n,
                                tile_w=tw, tile_h=th, view=_view(shot))
            mine = _mine(w, h, k, n, tw, th)
            assert 0 < mine.sum() < w * h and st["samples"] == int(mine.sum()) * SPP
            assert not part[~mine].any()
            total += part
            seen += mine
        assert (seen == 1).all()
        assert view_ref.same_bits(total, ref32) == 0
    # features of one shard (host variant): the other records stay empty
    feat = r.features(_cam(shot, 0.05, w, h), w, h, shard_index=1, shard_count=n, tile=(tw, th), view=_view(shot))
    full = _features_ref(st_.arrays, _rcam(shot, 0.0, w, h), SHOTS[shot][3], r.trace)
    mine = _mine(w, h, 1, n, tw, th)
    none = np.zeros(1, dtype=pt.FEATURE)
    none["prim"] = -1
    assert feat[mine].tobytes() == full[mine].tobytes()
    assert feat[~mine].tobytes() == none.tobytes() * int((~mine).sum())
    assert (full[mine]["prim"] >= 0).sum() > 0


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("shot", CONSUMER_SHOTS)
def test_accumulator_in_morton_order(stages, shot, integ):
    st_ = stages("cornell")
    n = 16
    ref32 = np.asarray(st_.ref(shot, 0.05, integ, n, n)[0]).astype(F)
    want = np.zeros((n * n, 3), dtype=F)
    for y in range(n):
        for x in range(n):
            want[view_ref.morton(x, y)] = ref32[y, x]
    with st_.renderer().accumulator(_cam(shot, 0.05, n, n), n, n, BOUNCES, integ, SEED, pixel_order=pt.PT_ORDER_MORTON,
                                    view=_view(shot)) as acc:
        acc.add(2)
        acc.add(1)
        assert view_ref.same_bits(acc.image(), want) == 0


# pass_spp, max_samples, tol, min_batches.  (On the CPU restatement -- adaptive_ref.simulate over view_ref renders --
# tol 0.5 freezes 262 to 333 of the 384 pixels at 4 samples for both shots and integrators: no need to raise it.)
LOOP = dict(pass_spp=2, max_samples=8, tol=0.5, min_batches=2)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("shot", CONSUMER_SHOTS)
@pytest.mark.parametrize("loop", ["add_until", "add_adaptive"])
def test_convergence_loops(stages, loop, shot, integ):
    st_ = stages("cornell")
    with st_.renderer().accumulator(_cam(shot, 0.0), W, H, BOUNCES, integ, SEED, view=_view(shot)) as acc:
        res = getattr(acc, loop)(LOOP["pass_spp"], LOOP["max_samples"], tol=LOOP["tol"], min_batches=LOOP["min_batches"])
        counts, mean, samples = acc.counts(), acc.mean64(), acc.samples
        active = np.zeros(W * H, dtype=bool)
        active[acc.active_pixels()] = True
        active = active.reshape(H, W)
    print(loop, shot, integ, "passes", res["passes"], "samples", samples, "counts",
          dict(zip(*[a.tolist() for a in np.unique(counts, return_counts=True)])))
    assert 2 * LOOP["pass_spp"] <= samples <= LOOP["max_samples"] and res["passes"] * LOOP["pass_spp"] == samples
    assert (counts[active] == samples).all()                     # every active pixel has every pass
    assert (counts >= LOOP["pass_spp"] * LOOP["min_batches"]).all() and (counts <= samples).all()
    if loop == "add_until":
        assert active.all() and (counts == samples).all()
    else:
        assert (counts < LOOP["max_samples"]).any() and (~active).any()          # some pixel froze below the maximum
        assert ((counts < samples) <= ~active).all()
    ref = view_ref.render(st_.osc, _rcam(shot, 0.0), SHOTS[shot][3], 0, BOUNCES, integ, SEED, counts=counts)
    assert view_ref.same_bits(mean, ref) == 0


@pytest.mark.parametrize("shot", CONSUMER_SHOTS)
def test_group_of_several_ranks(stages, shot):
    import torch
    n = min(torch.cuda.device_count(), 4)
    if n < 2:
        pytest.skip("one visible device (test_gpu_view.py has the one-rank group)")
    st_ = stages("cornell")
    rs = [st_.renderer()] + [pt.Renderer(st_.scene, d) for d in range(1, n)]
    try:
        with pt.Group(rs) as g:
            for integ in (0, 1):
                img, st = g.render(_cam(shot, 0.05), W, H, SPP, BOUNCES, integ, SEED, view=_view(shot))
                one, _ = rs[0].render(_cam(shot, 0.05), W, H, SPP, BOUNCES, integ, SEED, view=_view(shot))
                assert view_ref.same_bits(img, one) == 0
                _check(st_, img, st, shot, 0.05, integ, what="group of %d" % n)
    finally:
        for r in rs[1:]:
            r.close()
