"""Caller-built scenes on every walk, GPU against the CPU oracle on the same arrays, bit for bit.

pt_create takes the caller's own reference BVH.  The scenes of caller_scenes.py keep a fixture's triangles and hand
over trees the library's builder never makes: children exchanged (the other copy of an exact duplicate wins), a median
split numbered depth-first, shuffled node arrays (children before their parents), boxes looser than the vertices
(within the Markstein range, and with coordinates beyond 2^20), an overstated bvh_depth, chains of depth 63, and scene
lists written another way (shared and unused vertices, flipped and scaled normals, interleaved sphere and triangle
lights, the light area summed in another order).  Nothing here compares one GPU path with another: the oracle walks the
same tree, so its winner among equal distances depends on the tree exactly as the device's must.

Depth 63.  Every stack is sized from bvh_depth + 2 entries (DESIGN.md "Stack bounds"): pt_render's tile kernel needs
(63 + 2) * 512 B = 33 280 B of LDS per block, pt_trace / pt_trace_device with PT_FLAG_REFERENCE_BVH (63 + 2) * 1024 B =
66 560 B; the refusal (PT_E_BVH_DEPTH) starts at 160 KiB, i.e. at bvh_depth 319 and 159, beyond the 63 pt_create
accepts.  So no entry point refuses depth 63: the largest depth every entry point accepts is 63 as well, and the chains
run on all of them.  (tests/test_caller_scenes_host.py holds every refusal; no invalid tree reaches a kernel.)"""
import numpy as np
import pytest

import cudapathtracer_amd as pt

import caller_scenes as cs
import denoise_ref
import jitter_ref
import query_cases as qc
import view_ref
from test_gpu_query import check_closest, check_occluded, occ_dev

pytestmark = pytest.mark.gpu

F = np.float32
N = 5000
W, H, SPP, BOUNCES, SEED = 32, 24, 4, 3, 1234
POS = (0.0, 1.0, 3.0)
BASES = ("cornell", "soup", "cornell_spheres")
BUILDERS, CHAINS = cs.BUILDER_NAMES, cs.CHAIN_NAMES
KEYS = [(b, k) for b in BASES for k in BUILDERS] + [("subset", k) for k in CHAINS]
RENDER_FLAGS = (0, pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_REFERENCE_BVH)


def _cam():
    return pt.make_camera(POS, 1.0, 3.0, 0.0, W, H)


RCAM = (POS, 1.0, 3.0, 0.0, W, H)      # the same camera as view_ref / jitter_ref take it


class Case:
    """One caller-built scene: its renderer, its oracle scene and the oracle's answers (each computed once)."""

    def __init__(self, key, arrays):
        import oracle
        self.key, self.arrays = key, arrays
        assert cs.check_contract(arrays) == [], key      # (never an invalid tree on the GPU)
        self.scene = cs.ArrayScene(arrays)
        self.osc = oracle.OracleScene(arrays)
        self.renderer = pt.Renderer(self.scene, 0)
        self._img, self._sets = {}, None

    def trace(self, o, d):
        import oracle
        return oracle.trace_batch(self.osc, o, d)

    def ref(self, integ):
        import oracle
        if integ not in self._img:
            img, cnt = oracle.render(self.osc, oracle.camera(POS, 1.0, 3.0, 0.0, W, H), W, H, SPP, BOUNCES, integ, SEED)
            img.setflags(write=False)
            self._img[integ] = (img, cnt)
        return self._img[integ]

    def sets(self):
        if self._sets is None:
            sets = cs.ray_sets(self.arrays, N, 9, self.trace)
            self._sets = {k: (o, d, *self.trace(o, d)) for k, (o, d) in sets.items()}
        return self._sets


@pytest.fixture(scope="module")
def all_arrays(tmp_path_factory):
    soup = cs.load_soup(str(tmp_path_factory.mktemp("caller_soup")))
    bases = {"cornell": cs.load_cornell(), "soup": soup, "cornell_spheres": cs.load_cornell(True)}
    out = {(b, k): a for b in BASES for k, a in cs.builders(bases[b]).items()}
    out.update({("subset", k): a for k, a in cs.builders(cs.soup_subset(soup), chains=True).items()})
    assert sorted(out) == sorted(KEYS)
    glow = cs.glowing(soup)
    out.update({("glow", "library"): glow, ("glow", "swapped"): cs.swapped(glow), ("glow", "median"): cs.median(glow),
                ("glow", "permuted"): cs.permuted(glow, 1)})
    return out


@pytest.fixture(scope="module")
def cases(all_arrays):
    made = {}

    def get(key):
        if key not in made:
            made[key] = Case(key, all_arrays[key])
        return made[key]
    yield get
    for c in made.values():
        c.renderer.close()


@pytest.fixture(params=KEYS, ids=lambda k: "%s-%s" % k)
def case(request, cases):
    return cases(request.param)


def _bits(img, ref64):
    return int(np.count_nonzero(np.ascontiguousarray(img).view(np.uint32) != ref64.astype(F).view(np.uint32)))


# ---------------------------------------------------------------- trace and queries
def test_trace_and_queries_equal_the_oracle(case):
    """pt_trace and pt_trace_device on both walks, pt_occluded_device (and pt_occluded) with the tmax classes of
    query_cases.py and unbounded: 5000 rays per set; every set hits in at least a quarter of its rays."""
    r = case.renderer
    sets = case.sets()
    assert set(sets) == {"interior", "tiny", "bounce", "vertices", "zero", "far"}
    for j, (name, (o, d, etri, et)) in enumerate(sets.items()):
        assert len(o) >= (N if name != "bounce" else N // 4)
        assert 4 * np.count_nonzero(etri >= 0) >= len(o), (case.key, name, int(np.count_nonzero(etri >= 0)))
        check_closest(r, o, d, etri, et, (case.key, name))
        check_occluded(r, o, d, etri, et, j, (case.key, name))
        assert occ_dev(r, o, d, None).tobytes() == qc.expected_occ(etri, et, None).tobytes(), (case.key, name)
    o, d = sets["zero"][:2]
    assert ((d == 0).sum(axis=1) >= 1).all() and ((d == 0).sum(axis=1) == 2).any()
    o, d = sets["far"][:2]
    # beyond 64 extents of the geometry, however wide the caller's root box: the reference's own walk, its stack in
    # the lane's memory column (test_far_origins_take_the_reference_walk_whatever_the_root_box shows which walk ran)
    assert not qc.ray_regular(case.arrays, o, d).any()
    o, d = sets["tiny"][:2]
    assert not qc.ray_fast(o, d).all()


# ---------------------------------------------------------------- renders
@pytest.mark.parametrize("integ", [0, 1])
def test_renders_equal_the_oracle(case, integ):
    """The wavefront kernel, the tile kernel in the reference's traversal order and the reference-BVH walk; the
    default path also as three shards summed.  rays_reference is the oracle's trace count."""
    ref, cnt = case.ref(integ)
    for flags in RENDER_FLAGS:
        img, st = case.renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=integ, seed=SEED, flags=flags)
        assert _bits(img, ref) == 0, (case.key, integ, flags, _bits(img, ref))
        assert st["rays_reference"] == cnt["traces"] and st["samples"] == W * H * SPP
        if flags == 0 and case.key[0] != "subset":
            # which walk ran (pt_stats.accel_fallbacks, the rays that took the exact slow walk): all of them when a
            # box coordinate leaves the Markstein range, almost none otherwise -- looser boxes make the reference test
            # more triangles, never fewer, so the winner check fails no more often than on the tight tree, for which
            # tests/test_gpu_parity.py sets this bound
            print(case.key, integ, "rays_traced", st["rays_traced"], "accel_fallbacks", st["accel_fallbacks"])
            if case.key[1] == "loose_big":
                assert st["accel_fallbacks"] == st["rays_traced"] > 0
            elif case.key[1] in ("library", "loose", "loose_root"):
                assert st["accel_fallbacks"] <= max(10, st["rays_traced"] // 10000)
    assert np.isfinite(img).all() and np.count_nonzero(img) > 0
    acc = np.zeros((H, W, 3), dtype=F)
    rays = 0
    for k in range(3):
        part, st = case.renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=integ, seed=SEED, shard_index=k,
                                        shard_count=3)
        acc += part
        rays += st["rays_reference"]
    assert _bits(acc, ref) == 0 and rays == cnt["traces"]


# ---------------------------------------------------------------- the other paths
def test_features_equal_the_host_composition(case):
    got = case.renderer.features(_cam(), W, H)
    want = denoise_ref.features_ref(case.arrays, _cam(), W, H, case.trace)
    assert np.count_nonzero(want["prim"] >= 0) > W * H // 8
    assert got.tobytes() == want.tobytes()


def test_accumulated_passes(case):
    """Two adds equal one render of the sum; the f64 mean is the oracle's."""
    ref, cnt = case.ref(0)
    with case.renderer.accumulator(_cam(), W, H, bounces=BOUNCES, integrator=0, seed=SEED) as acc:
        rays = acc.add(3)["rays_reference"] + acc.add(1)["rays_reference"]
        img, mean = acc.image(), acc.mean64()
    assert mean.tobytes() == ref.tobytes()
    assert _bits(img, ref) == 0 and rays == cnt["traces"]


def test_oriented_view_and_jitter(case):
    """One look-at render and one jittered render (tent filter), against the restated loops of view_ref / jitter_ref
    over the oracle's integrators."""
    v = view_ref.generic(POS)
    want, cnt = view_ref.render(case.osc, RCAM, v, SPP, BOUNCES, 0, SEED, return_counters=True)
    img, st = case.renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=0, seed=SEED, view=pt.make_view(*v))
    assert _bits(img, want) == 0 and st["rays_reference"] == cnt["traces"]
    assert np.count_nonzero(img) > 0
    flags = pt.PT_FLAG_JITTER | pt.PT_FLAG_JITTER_TENT
    want, cnt = jitter_ref.render(case.osc, RCAM, None, flags, SPP, BOUNCES, 1, SEED, return_counters=True)
    img, st = case.renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=1, seed=SEED, flags=flags)
    assert _bits(img, want) == 0 and st["rays_reference"] == cnt["traces"]
    assert np.count_nonzero(img) > 0


# ---------------------------------------------------------------- the image follows the caller's tree
def test_image_depends_on_the_tree_only_where_the_oracle_says_so(cases):
    """Trees over the same triangles give the same image exactly where the oracle's images are the same (in Cornell
    rays through shared edges tie, so even there the tree shows).  On the soup with every material glowing, the exact
    duplicates under other materials make the oracle's image differ once the children are exchanged, and so must the
    device's: a kernel that ignored the caller's tree could not pass."""
    trees = ("library", "swapped", "median", "permuted")
    for integ in (0, 1):
        for base in ("cornell", "glow"):
            want = {k: cases((base, k)).ref(integ)[0].astype(F) for k in trees}
            got = {k: cases((base, k)).renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=integ, seed=SEED)[0]
                   for k in trees}
            for k in trees:
                assert got[k].tobytes() == want[k].tobytes(), (base, k, integ)
                for k2 in trees:
                    assert (got[k].tobytes() == got[k2].tobytes()) == (want[k].tobytes() == want[k2].tobytes())
        differ = int(np.count_nonzero((want["library"] != want["swapped"]).any(axis=2)))
        print("glowing soup, integrator %d: the oracle's images differ in %d pixels" % (integ, differ))
        assert differ >= 1
        assert int(np.count_nonzero((got["library"] != got["swapped"]).any(axis=2))) == differ
        for k in ("median", "permuted"):            # the same tie order as the library's tree: the same image
            assert want[k].tobytes() == want["library"].tobytes()


def _far_cam(z):
    """On the +z axis at distance z, looking down -z, the field of view narrowed so that the scene fills the frame."""
    import oracle
    kw = dict(pos=(0.0, 1.0, float(z)), dist_from_film=float(z) / 3.0, focal_length=float(z), radius=0.0)
    return (pt.make_camera(width=W, height=H, **kw), oracle.camera(kw["pos"], kw["dist_from_film"], kw["focal_length"], 0.0, W, H))


@pytest.mark.parametrize("key", [("soup", "loose_root"), ("cornell_spheres", "loose_root"), ("soup", "library")],
                         ids=lambda k: "%s-%s" % k)
def test_far_origins_take_the_reference_walk_whatever_the_root_box(cases, key):
    """The BVH4 boxes' margin covers the conservative box test up to origins 64 extents of the geometry out
    (pt_device.h ray_regular); beyond, a ray must take the reference's own walk.  A caller's root box 2^19 wide around
    geometry a few units across must not move that bound: origins between 64 geometry extents and 64 root-box extents
    give the oracle's bits, and the per-triangle test counts (kernel.cu:133) say which walk ran -- the reference's walk
    tests exactly the triangles the oracle tests, the culled BVH4 walk far fewer (shown on the interior set).  Whole
    renders and the features from a camera in that range take the tile kernel's reference-BVH walk (no work units)."""
    import oracle
    c = cases(key)
    ext = float(cs.geometry_extent(c.arrays))
    root = float(np.abs(np.stack([c.arrays["bvh"]["lo"][0], c.arrays["bvh"]["hi"][0]])).max())
    assert ext < 7 and (root == cs.WIDE if key[1] == "loose_root" else root <= ext)
    o, d, etri, et = c.sets()["far"]
    far = np.abs(o).max(axis=1)
    assert far.min() > 64 * ext and far.max() < 64 * float(cs.WIDE)
    assert 4 * np.count_nonzero(etri >= 0) >= len(o)
    for name, reference_walk in (("far", True), ("interior", False)):
        o, d, etri, et = c.sets()[name]
        tri, t, counts, _ = c.renderer.trace_counts(o, d, reference_bvh=False)
        assert np.array_equal(tri, etri) and t.tobytes() == et.tobytes(), (key, name)
        want = np.zeros(len(c.arrays["tris"]), dtype=np.uint32)
        oracle.trace_batch(c.osc, o, d, tri_counts=want)
        print(key, name, "triangle tests: device %d, oracle %d" % (counts.sum(), want.sum()))
        if reference_walk:
            assert np.array_equal(counts, want) and want.sum() > 0, (key, name)
        else:
            assert counts.sum() < want.sum(), (key, name)
    z = 500.0
    assert 64 * ext < z < 64 * float(cs.WIDE)
    cam, ocam = _far_cam(z)
    for integ in (0, 1):
        ref, cnt = oracle.render(c.osc, ocam, W, H, SPP, BOUNCES, integ, SEED)
        assert np.count_nonzero(ref.astype(F).max(axis=2) > 0) > W * H // 32
        img, st = c.renderer.render(cam, W, H, SPP, bounces=BOUNCES, integrator=integ, seed=SEED)
        assert _bits(img, ref) == 0 and st["rays_reference"] == cnt["traces"], (key, integ)
        assert st["work_units"] == 0, (key, integ)          # (not the wavefront kernel: the camera is far)
    want = denoise_ref.features_ref(c.arrays, cam, W, H, c.trace)
    assert np.count_nonzero(want["prim"] >= 0) > W * H // 8
    assert c.renderer.features(cam, W, H).tobytes() == want.tobytes()


def test_depth_63_is_accepted_by_every_entry_point(cases):
    """The sizing sites (pt_render_host.h): the refusals start at bvh_depth 159 (pt_trace, the queries) and 319
    (pt_render), so at 63 nothing refuses; the walks of a left-leaning chain fill their stacks to the tree's depth."""
    c = cases(("subset", "chain_left"))
    assert c.arrays["bvh_depth"] == 63 == cs.true_depth(c.arrays["bvh"])
    o, d, etri, et = c.sets()["far"]
    tri, t, counts, spills = c.renderer.trace_counts(o, d, reference_bvh=True)
    assert np.array_equal(tri, etri) and t.tobytes() == et.tobytes()
    want = np.zeros(len(c.arrays["tris"]), dtype=np.uint32)
    import oracle
    oracle.trace_batch(c.osc, o, d, tri_counts=want)
    assert np.array_equal(counts, want) and counts.sum() > 0      # the same triangles tested: the same walk
    img, st = c.renderer.render(_cam(), W, H, SPP, bounces=BOUNCES, integrator=0, seed=SEED,
                                flags=pt.PT_FLAG_REFERENCE_TRAVERSAL | pt.PT_FLAG_COUNT)
    assert _bits(img, c.ref(0)[0]) == 0
