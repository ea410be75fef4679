"""Every *_device entry point inside guard bands (tests/guard_bands.py): each device buffer a call takes is the payload
of an Arena, [front guard | payload | back guard], so a store outside a buffer changes a guard byte and a load from
outside an input reads a chosen poison.  Each case asserts

  1. every guard of every buffer is intact after the call, outputs and inputs alike;
  2. input payloads are unchanged (unless the call is run in place);
  3. the output payload is the same under both placements and both input poisons;
  4. the output payload equals, in every bit, the reference the entry point's own test uses at those arguments -- the
     oracle (oracle.render / trace_batch, directly or through view_ref, rays_ref, irradiance_ref), or the numpy
     restatements denoise_ref, denoise_guided_ref, temporal_ref, noise_ref / adaptive_ref, lightmap_ref, query_cases,
     pt.tonemap_u8 -- never another run of the library; pixels of other shards inside the payload keep 0xA5.

(3) is asserted twice over: every case is compared with the one cached reference, and with the bytes the earlier
cases of the same arguments produced (_seen).  Entry points without an input buffer have no poison to vary.  The scene
is cornell_blob with a diffuse and an emissive sphere; renders take 2 samples per pixel and 3 bounces.

The last test covers the context's grow-on-demand scratch instead: small after large with different data."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, rays, shard

import adaptive_ref
import denoise_guided_ref
import denoise_ref
import guard_bands as gb
import irradiance_ref
import lightmap_ref as lr
import noise_ref
import query_cases as qc
import rays_accum_ref
import rays_ref
import raysets
import temporal_ref
import view_ref
from guard_bands import Arena
from test_gpu_denoise import direct_gather

pytestmark = pytest.mark.gpu

F = np.float32
POS = (0.0, 1.0, 3.0)
SPP, BOUNCES, SEED = 2, 3, 1234
LOOK = temporal_ref.orbit_pose(3)                     # (pos, view) of the oriented camera
# (w, h, pixel order): one pixel; a partial 64-wide block and partial 8 x 8 tiles; one column and one row past a
# 64 x 32 tile; and the Morton order, which needs a power-of-two square
SHAPES = [(1, 1, 0), (37, 19, 0), (65, 33, 0), (32, 32, 1)]
SCAN_SHAPES = [s for s in SHAPES if not s[2]]
MODES = [(0, 0, 1), (1, 0, 1), (0, 0, 2), (1, 1, 2)]  # (integrator, shard_index, shard_count), the default 8 x 8 tile
SHARDS = [(0, 1), (0, 2), (1, 2)]
KERNELS = {"default": (False, None), "direct": (True, None), "tiled16": (False, 16)}   # test_gpu_denoise.direct_gather

shape_ids = lambda s: "%dx%d%s" % (s[0], s[1], "m" if s[2] else "")
on_shapes = pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
on_scan_shapes = pytest.mark.parametrize("shape", SCAN_SHAPES, ids=shape_ids)
on_placements = pytest.mark.parametrize("placement", gb.PLACEMENTS)
on_poisons = pytest.mark.parametrize("poison", gb.POISONS, ids=lambda p: "poison%02x" % p)


# ---------------------------------------------------------------- the scene, its oracle and the cached references
class Stage:
    def __init__(self):
        import oracle
        self.oracle = oracle
        self.scene = load_scene("cornell_blob")
        self.scene.add_sphere((0.4, 0.3, 0.5), 0.3, (0.6, 0.7, 0.8))
        self.scene.add_sphere((-0.5, 0.25, 0.6), 0.25, (0.5, 0.5, 0.5), (3.0, 3.0, 3.0))
        self.arrays = self.scene.arrays()
        self.nt = int(self.arrays["tris"].shape[0])
        self.osc = oracle.OracleScene(self.arrays)
        self.r = pt.Renderer(self.scene, 0)
        self.cache = {}

    def trace(self, o, d):
        return self.oracle.trace_batch(self.osc, o, d)

    def ref(self, key, make):
        if key not in self.cache:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.cache[key] = v
        return self.cache[key]


@pytest.fixture(scope="module")
def st():
    s = Stage()
    yield s
    s.r.close()


def _cam(w, h, pos=POS):
    return pt.make_camera(pos, 1.0, 3.0, 0.0, w, h)


def _view(v=LOOK[1]):
    return pt.make_view(v[0], v[1], v[2], v[3])


def _midx(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return shard.morton_index(xx, yy).astype(np.int64).reshape(-1)


def _ordered(a, w, h, order):
    """A scanline (h, w, ...) or (h*w, ...) array as (w*h, ...) rows in the pixel order the library takes."""
    a = np.asarray(a)
    a = a.reshape((w * h,) + a.shape[(2 if a.shape[:2] == (h, w) else 1):])
    if not order:
        return np.ascontiguousarray(a)
    out = np.empty_like(a)
    out[_midx(w, h)] = a
    return out


def _mine(w, h, k, n, order):
    """The mask, in pixel order, of the pixels shard k of n owns (default tile)."""
    m = np.zeros(w * h, dtype=bool)
    m[shard.shard_pixels(w, h, k, n)] = True
    return _ordered(m.reshape(h, w), w, h, order)


def _rows(w, h, order, scan_rows):
    """Rows given in scanline order ((w*h, k) float32: rays, points) in the library's pixel order."""
    return _ordered(np.ascontiguousarray(scan_rows).reshape(h, w, -1), w, h, order)


def _cam_mean(st, w, h, n, integ):
    ocam = st.oracle.camera(POS, 1.0, 3.0, 0.0, w, h)
    return st.ref(("cam", w, h, n, integ), lambda: st.oracle.render(st.osc, ocam, w, h, n, BOUNCES, integ, SEED)[0])


def _view_mean(st, w, h, n, integ):
    return st.ref(("view", w, h, n, integ),
                  lambda: view_ref.render(st.osc, (LOOK[0], 1.0, 3.0, 0.0, w, h), LOOK[1], n, BOUNCES, integ, SEED))


def _ray_set(st, w, h):
    """Scanline (w*h, 6) rays: an orthographic set, a distinct origin per pixel."""
    return st.ref(("rays", w, h), lambda: np.concatenate(rays_ref.set_ortho(w, h), axis=1).astype(F))


def _ray_mean(st, w, h, n, integ):
    rs = _ray_set(st, w, h)
    return st.ref(("raymean", w, h, n, integ),
                  lambda: rays_ref.render(st.osc, rs[:, :3], rs[:, 3:], w, h, n, BOUNCES, integ, SEED))


def _point_set(st, w, h):
    return st.ref(("points", w, h), lambda: np.concatenate(irradiance_ref.set_floor(w, h), axis=1).astype(F))


def _point_mean(st, w, h, n, integ):
    ps = _point_set(st, w, h)
    return st.ref(("pointmean", w, h, n, integ),
                  lambda: irradiance_ref.render(st.osc, ps[:, :3], ps[:, 3:], w, h, n, BOUNCES, integ, SEED))


MEANS = {"camera": _cam_mean, "rays": _ray_mean, "points": _point_mean}


def _features(st, w, h, kind, pose=None):
    """Scanline (h, w) feature records composed on the host from the oracle's trace: of the reference camera
    (denoise_ref.features_ref), of the oriented camera at `pose` (view_ref.rays), of the ray set."""
    if kind == "camera":
        return st.ref(("feat", w, h), lambda: denoise_ref.features_ref(st.arrays, _cam(w, h), w, h, st.trace))
    if kind == "rays":
        rs = _ray_set(st, w, h)
        return st.ref(("featrays", w, h), lambda: rays_accum_ref.features_ref(st.arrays, rs[:, :3], rs[:, 3:], w, h, st.trace))
    pose = LOOK if pose is None else pose

    def make():
        ys, xs = np.mgrid[0:h, 0:w]
        o, d = view_ref.rays((pose[0], 1.0, 3.0, 0.0, w, h), pose[1], xs.reshape(-1), ys.reshape(-1), False)
        return rays_accum_ref.features_ref(st.arrays, o, d, w, h, st.trace)
    return st.ref(("featview", w, h, pose[0]), make)


# ---------------------------------------------------------------- arenas of one call, and the comparisons
class Bands:
    def __init__(self, placement, poison=None):
        self.placement, self.poison = placement, poison
        self.arenas, self.inputs = [], []

    def out(self, nbytes, align):
        a = Arena(nbytes, align, gb.OUT_FILL, "cuda", self.placement)
        a.fill_payload(gb.OUT_FILL)
        self.arenas.append(a)
        return a

    def inp(self, array, align, in_place=False):
        """An input's arena, its guards poisoned; in_place: the call may write the payload (it is the output too)."""
        array = np.ascontiguousarray(array)
        a = Arena(array.nbytes, align, self.poison, "cuda", self.placement).load(array)
        self.arenas.append(a)
        if not in_place:
            self.inputs.append((a, array.tobytes()))
        return a

    def ready(self):
        torch.cuda.synchronize()
        return self

    def verify(self, what):
        torch.cuda.synchronize()
        for k, a in enumerate(self.arenas):
            assert a.guards_intact(), "%s: buffer %d: %s" % (what, k, a.describe())
        for a, want in self.inputs:
            assert a.payload_bytes() == want, "%s: an input payload changed" % (what,)


def _same(got, want, what):
    g = np.frombuffer(np.ascontiguousarray(got).tobytes(), dtype=np.uint8)
    w = np.frombuffer(np.ascontiguousarray(want).tobytes(), dtype=np.uint8)
    assert g.size == w.size, (what, g.size, w.size)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d bytes differ from the reference, the first at byte %d, the last at byte %d" % (
        what, bad.size, g.size, bad[0], bad[-1])


_SEEN = {}


def _seen(key, got):
    """The same arguments under another placement or poison gave the same bytes."""
    b = np.ascontiguousarray(got).tobytes()
    assert _SEEN.setdefault(key, b) == b, "%s: differs from the run under another placement or poison" % (key,)


def _shard_expect(ref_rows, mine, held=None):
    """What a shard's call leaves in a buffer of w*h rows: the reference on the shard's rows, on the others what the
    buffer held (0xA5 bytes when fresh)."""
    ref_rows = np.ascontiguousarray(ref_rows)
    out = np.frombuffer(bytes([gb.OUT_FILL]) * ref_rows.nbytes, dtype=ref_rows.dtype).reshape(ref_rows.shape).copy() \
        if held is None else np.array(held, copy=True)
    out[mine] = ref_rows[mine]
    return out


def _params(w, h, order, integ=0, k=0, n=1, spp=SPP):
    return pt.Renderer.params(w, h, spp, BOUNCES, integ, SEED, 0, k, n, order)


def _sptr(s):
    return None if s is None else C.c_void_p(int(s))


# ---------------------------------------------------------------- 1. renders: d_out
@on_placements
@on_shapes
@pytest.mark.parametrize("entry", ["pt_render_device", "pt_render_device_view"])
def test_render_device(st, entry, shape, placement):
    w, h, order = shape
    L = _lib.lib()
    for integ, k, n in MODES:
        b = Bands(placement)
        out = b.out(w * h * 12, 4)
        b.ready()
        stats = _lib.Stats()
        p = _params(w, h, order, integ, k, n)
        if entry == "pt_render_device":
            _lib.check(L.pt_render_device(st.r._h, C.byref(p), C.byref(_cam(w, h)), C.c_void_p(out.ptr), None, C.byref(stats)))
            ref = _cam_mean(st, w, h, SPP, integ)
        else:
            _lib.check(L.pt_render_device_view(st.r._h, C.byref(p), C.byref(_cam(w, h, LOOK[0])), C.byref(_view()),
                                               C.c_void_p(out.ptr), None, C.byref(stats)))
            ref = _view_mean(st, w, h, SPP, integ)
        what = (entry, shape, placement, integ, k, n)
        b.verify(what)
        mine = _mine(w, h, k, n, order)
        assert stats.samples == int(mine.sum()) * SPP, what
        got = out.read(F, (w * h, 3))
        _same(got, _shard_expect(_ordered(ref.astype(F), w, h, order), mine), what)
        _seen((entry, shape, integ, k, n), got)


@on_placements
@on_shapes
def test_render_device_async_two_in_flight(st, shape, placement):
    """pt_render_device_async + pt_render_wait: two renders in flight into two arenas on two streams, both collected
    before anything is read."""
    w, h, order = shape
    L = _lib.lib()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for pair in (MODES[:2], MODES[2:]):
        b = Bands(placement)
        outs = [b.out(w * h * 12, 4), b.out(w * h * 12, 4)]
        b.ready()
        for (integ, k, n), out, s in zip(pair, outs, streams):
            p = _params(w, h, order, integ, k, n)
            _lib.check(L.pt_render_device_async(st.r._h, C.byref(p), C.byref(_cam(w, h)), C.c_void_p(out.ptr), _sptr(s.cuda_stream)))
        stats = [st.r.wait(), st.r.wait()]
        b.verify(("async", shape, placement, pair))
        for (integ, k, n), out, s in zip(pair, outs, stats):
            mine = _mine(w, h, k, n, order)
            assert s["samples"] == int(mine.sum()) * SPP
            got = out.read(F, (w * h, 3))
            _same(got, _shard_expect(_ordered(_cam_mean(st, w, h, SPP, integ).astype(F), w, h, order), mine),
                  ("async", shape, placement, integ, k, n))
            _seen(("async", shape, integ, k, n), got)


# ---------------------------------------------------------------- 2. feature buffers: d_feat
@on_placements
@on_shapes
@pytest.mark.parametrize("entry", ["pt_render_features_device", "pt_render_features_view_device"])
def test_features_device(st, entry, shape, placement):
    w, h, order = shape
    L = _lib.lib()
    for k, n in SHARDS:
        b = Bands(placement)
        out = b.out(w * h * 48, 16)
        b.ready()
        p = pt.Renderer.params(w, h, 0, 1, 0, 0, 0, k, n, order)
        if entry == "pt_render_features_device":
            _lib.check(L.pt_render_features_device(st.r._h, C.byref(p), C.byref(_cam(w, h)), C.c_void_p(out.ptr), None))
            ref = _features(st, w, h, "camera")
        else:
            _lib.check(L.pt_render_features_view_device(st.r._h, C.byref(p), C.byref(_cam(w, h, LOOK[0])), C.byref(_view()),
                                                        C.c_void_p(out.ptr), None))
            ref = _features(st, w, h, "view")
        what = (entry, shape, placement, k, n)
        b.verify(what)
        got = out.read(pt.FEATURE, (w * h,))
        _same(got, _shard_expect(_ordered(ref, w, h, order), _mine(w, h, k, n, order)), what)
        _seen((entry, shape, k, n), got)
    if w * h > 1:
        assert (ref["prim"] >= st.nt).any() and (ref["prim"] < 0).any()        # a sphere and a miss are in view


# ---------------------------------------------------------------- 3. renders and features along rays, at points
@on_poisons
@on_placements
@on_shapes
@pytest.mark.parametrize("entry", ["pt_render_rays_device", "pt_render_irradiance_device"])
def test_render_rays_and_irradiance_device(st, entry, shape, placement, poison):
    w, h, order = shape
    L = _lib.lib()
    data, mean, call = (_ray_set, _ray_mean, L.pt_render_rays_device) if entry == "pt_render_rays_device" else \
        (_point_set, _point_mean, L.pt_render_irradiance_device)
    for integ, k, n in MODES:
        b = Bands(placement, poison)
        src = b.inp(_rows(w, h, order, data(st, w, h)), 8)
        out = b.out(w * h * 12, 4)
        b.ready()
        stats = _lib.Stats()
        p = _params(w, h, order, integ, k, n)
        _lib.check(call(st.r._h, C.byref(p), C.c_void_p(src.ptr), C.c_void_p(out.ptr), None, C.byref(stats)))
        what = (entry, shape, placement, poison, integ, k, n)
        b.verify(what)
        mine = _mine(w, h, k, n, order)
        assert stats.samples == int(mine.sum()) * SPP, what
        got = out.read(F, (w * h, 3))
        _same(got, _shard_expect(_ordered(mean(st, w, h, SPP, integ).astype(F), w, h, order), mine), what)
        _seen((entry, shape, integ, k, n), got)


@on_poisons
@on_placements
@on_shapes
def test_features_rays_device(st, shape, placement, poison):
    w, h, order = shape
    L = _lib.lib()
    ref = _ordered(_features(st, w, h, "rays"), w, h, order)
    for k, n in SHARDS:
        b = Bands(placement, poison)
        src = b.inp(_rows(w, h, order, _ray_set(st, w, h)), 8)
        out = b.out(w * h * 48, 16)
        b.ready()
        p = pt.Renderer.params(w, h, 0, 1, 0, 0, 0, k, n, order)
        _lib.check(L.pt_render_features_rays_device(st.r._h, C.byref(p), C.c_void_p(src.ptr), C.c_void_p(out.ptr), None))
        what = ("pt_render_features_rays_device", shape, placement, poison, k, n)
        b.verify(what)
        got = out.read(pt.FEATURE, (w * h,))
        _same(got, _shard_expect(ref, _mine(w, h, k, n, order)), what)
        _seen(("featrays", shape, k, n), got)


# ---------------------------------------------------------------- 4. the classes of rays and points: input only
def _class_sets(st, m):
    """name -> ((m, 6) rays or points, the restatement's classes): both sides of the bounds of pt.h's classes (raysets.
    regular_edge_sets), and the same with an invalid last entry -- the entry a read past the end would join."""
    ext = rays_ref.scene_extent(st.arrays)
    sets = raysets.regular_edge_sets(st.arrays, m, 5)
    out = {}
    o, d = sets["origin_bound"]
    o2, d2 = sets["dir_length"]
    bad = d2.copy()
    bad[m - 1] = 0
    for name, (a, c) in (("origin_bound", (o, d)), ("dir_length", (o2, d2)), ("invalid_last", (o2, bad))):
        out["rays/" + name] = (np.concatenate([a, c], axis=1).astype(F), rays_ref.classify(a, c, ext)[0])
    nrm = rays._normalised(sets["origin_bound"][1])
    badn = nrm.copy()
    badn[m - 1] = nrm[m - 1] * F(1.01)
    for name, (a, c) in (("origin_bound", (o, nrm)), ("invalid_last", (o, badn))):
        out["points/" + name] = (np.concatenate([a, c], axis=1).astype(F), irradiance_ref.classify(a, c, ext)[0])
    return out


@on_poisons
@on_placements
@on_scan_shapes
def test_classify_device(st, shape, placement, poison):
    """pt_rays_classify_device and pt_points_classify_device over w*h entries.  A read of one entry past the end would
    add an invalid one under either poison (a zero direction, a NaN)."""
    w, h, _ = shape
    m = w * h
    sets = st.ref(("classes", m), lambda: _class_sets(st, m))
    seen = dict(regular=0, irregular=0, invalid=0)
    for name, (rows, want) in sets.items():
        b = Bands(placement, poison)
        src = b.inp(rows, 8)
        b.ready()
        got = st.r.classify_rays_device(src.ptr, m) if name.startswith("rays/") else st.r.classify_points_device(src.ptr, m)
        b.verify((name, shape, placement, poison))
        assert got == want, (name, shape, placement, poison, got, want)
        for key in seen:
            seen[key] += want[key]
    assert seen["invalid"] == 2 and seen["regular"] > 0 and (m == 1 or seen["irregular"] > 0)


# ---------------------------------------------------------------- 5. ray queries
def _query_case(st, m):
    """(rays (m, 6), tri, t, tmax, occ with tmax, occ without) of the first m of a mix of query_cases' integrator sets."""
    sets = st.ref(("qsets",), lambda: qc.integrator_sets(st.arrays, 257, 31, st.trace))
    names = ("interior", "tiny", "outside", "axis", "bounce")
    i = np.arange(m)
    o = np.stack([sets[names[k % 5]][0][k % len(sets[names[k % 5]][0])] for k in i]).astype(F)
    d = np.stack([sets[names[k % 5]][1][k % len(sets[names[k % 5]][1])] for k in i]).astype(F)
    tri, t = st.trace(o, d)
    tm, _ = qc.tmax_cycle(t, 1)
    return np.concatenate([o, d], axis=1).astype(F), tri, t, tm, qc.expected_occ(tri, t, tm), qc.expected_occ(tri, t, None)


@on_poisons
@on_placements
@pytest.mark.parametrize("m", [1, 63, 65, 257])
def test_query_device(st, m, placement, poison):
    rows, tri, t, tm, occ, occ_any = st.ref(("query", m), lambda: _query_case(st, m))
    if m >= 63:
        assert (tri >= 0).any() and (tri < 0).any() and occ.any() and not occ.all()
    for ref_bvh in (False, True):
        b = Bands(placement, poison)
        src, d_tri, d_t = b.inp(rows, 8), b.out(m * 4, 4), b.out(m * 4, 4)
        b.ready()
        st.r.trace_device(src.ptr, m, d_tri.ptr, d_t.ptr, reference_bvh=ref_bvh)
        what = ("pt_trace_device", m, placement, poison, ref_bvh)
        b.verify(what)
        _same(d_tri.read(np.int32), tri, what)
        _same(d_t.read(F), t, what)
    for bound, want in ((tm, occ), (None, occ_any)):
        b = Bands(placement, poison)
        src, d_occ = b.inp(rows, 8), b.out(m, 1)
        d_tm = None if bound is None else b.inp(bound, 4)
        b.ready()
        st.r.occluded_device(src.ptr, m, d_occ.ptr, None if d_tm is None else d_tm.ptr)
        what = ("pt_occluded_device", m, placement, poison, bound is None)
        b.verify(what)
        _same(d_occ.read(np.uint8), want, what)


# ---------------------------------------------------------------- 6. accumulators
@on_poisons
@on_placements
@on_shapes
@pytest.mark.parametrize("kind", ["rays", "points"])
def test_accum_create_device(st, kind, shape, placement, poison):
    """pt_accum_create_rays_device / _points_device copy their input: the arena is read only, and what the accumulator
    then renders is the restatement's image of exactly those rays or points."""
    w, h, order = shape
    data, create = (_ray_set, st.r.accumulator_rays_device) if kind == "rays" else (_point_set, st.r.accumulator_points_device)
    for integ, k, n in MODES[1:3]:
        b = Bands(placement, poison)
        src = b.inp(_rows(w, h, order, data(st, w, h)), 8)
        b.ready()
        with create(src.ptr, w, h, BOUNCES, integ, SEED, 0, k, n, order) as acc:
            what = ("pt_accum_create_%s_device" % kind, shape, placement, poison, integ, k, n)
            b.verify(what)
            src.fill_payload(poison)                        # the accumulator holds its own copy
            acc.add(SPP)
            want = _ordered(MEANS[kind](st, w, h, SPP, integ).astype(F), w, h, order)
            want = np.where(_mine(w, h, k, n, order)[:, None], want, F(0))
            _same(acc.image().reshape(w * h, 3), want, what)


def _checker(w, h, order):
    return _ordered(rays_accum_ref.checkerboard(w, h), w, h, order)


def _until(render, shape, mine, pass_spp, cap, tol, quantile, min_batches):
    """pt_accum_add_until from 0 samples over render(n): the samples it stops at and whether it converged
    (noise_ref.NoiseRef and pt.h's rule)."""
    est = noise_ref.NoiseRef(0, shape=shape)
    samples, passes = 0, 0
    while samples < cap:
        samples += min(pass_spp, cap - samples)
        passes += 1
        est.update(samples, render(samples))
        s = est.summary(tol, noise_ref.Y_FLOOR, mine)
        if s["batches"] >= min_batches and s["converged"] >= int(np.ceil(np.float64(F(quantile)) * s["pixels"])):
            return samples, passes, True
    return samples, passes, False


# at the second pass some pixels converge and freeze, fewer than the quantile: the third samples the rest alone
LOOP = dict(pass_spp=1, max_samples=3, tol=0.5, quantile=0.95, min_batches=2)


def _make_acc(st, kind, w, h, order, integ, k, n):
    if kind == "camera":
        return st.r.accumulator(_cam(w, h), w, h, BOUNCES, integ, SEED, 0, k, n, order)
    rows = _rows(w, h, order, (_ray_set if kind == "rays" else _point_set)(st, w, h))
    make = st.r.accumulator_rays if kind == "rays" else st.r.accumulator_points
    return make(rows[:, :3], rows[:, 3:], w, h, BOUNCES, integ, SEED, 0, k, n, order)


@on_placements
@on_shapes
@pytest.mark.parametrize("kind", ["camera", "rays", "points"])
def test_accum_d_out(st, kind, shape, placement):
    """d_out of pt_accum_add, pt_accum_add_until and pt_accum_add_adaptive on a camera, a ray and a point accumulator:
    the shard's pixels hold the mean at their own counts, a frozen pixel what the buffer held, the rest 0xA5."""
    w, h, order = shape
    scan = lambda n, integ: MEANS[kind](st, w, h, n, integ)                             # f64 (h, w, 3), scanline
    for integ, k, n in MODES[1:]:
        mine = _mine(w, h, k, n, order)
        mean32 = lambda c: _ordered(scan(c, integ).astype(F), w, h, order)
        tag = (kind, shape, placement, integ, k, n)
        # add; freeze a checkerboard; add: frozen pixels keep what d_out held
        b = Bands(placement)
        out = b.out(w * h * 12, 4)
        b.ready()
        with _make_acc(st, kind, w, h, order, integ, k, n) as acc:
            acc.add(2, d_out_ptr=out.ptr)
            b.verify(("pt_accum_add",) + tag)
            first = out.read(F, (w * h, 3))
            _same(first, _shard_expect(mean32(2), mine), ("pt_accum_add",) + tag)
            frozen = _checker(w, h, order)
            acc.freeze(frozen)
            s = acc.add(1, d_out_ptr=out.ptr)
            b.verify(("pt_accum_add, frozen",) + tag)
            assert s["samples"] == int((mine & ~frozen).sum())
            got = out.read(F, (w * h, 3))
            _same(got, _shard_expect(mean32(3), mine & ~frozen, held=first), ("pt_accum_add, frozen",) + tag)
            _seen(("add",) + tag[:2] + tag[3:], got)
        # add_until
        mine_scan = _mine(w, h, k, n, 0).reshape(h, w)
        b = Bands(placement)
        out = b.out(w * h * 12, 4)
        b.ready()
        with _make_acc(st, kind, w, h, order, integ, k, n) as acc:
            res = acc.add_until(LOOP["pass_spp"], LOOP["max_samples"], LOOP["tol"], LOOP["quantile"], LOOP["min_batches"],
                                d_out_ptr=out.ptr)
            b.verify(("pt_accum_add_until",) + tag)
            got = out.read(F, (w * h, 3))
            if mine.any():
                samples, passes, conv = _until(lambda c: scan(c, integ), (h, w), mine_scan, LOOP["pass_spp"], LOOP["max_samples"],
                                               LOOP["tol"], LOOP["quantile"], LOOP["min_batches"])
                assert (res["samples"], res["passes"], res["stopped_converged"]) == (samples, passes, conv), tag
                _same(got, _shard_expect(mean32(samples), mine), ("pt_accum_add_until",) + tag)
            else:
                _same(got, _shard_expect(mean32(1), mine), ("pt_accum_add_until",) + tag)      # untouched
            _seen(("until",) + tag[:2] + tag[3:], got)
        # add_adaptive
        b = Bands(placement)
        out = b.out(w * h * 12, 4)
        b.ready()
        with _make_acc(st, kind, w, h, order, integ, k, n) as acc:
            res = acc.add_adaptive(LOOP["pass_spp"], LOOP["max_samples"], LOOP["tol"], LOOP["quantile"], LOOP["min_batches"],
                                   d_out_ptr=out.ptr)
            b.verify(("pt_accum_add_adaptive",) + tag)
            got = out.read(F, (w * h, 3))
            if mine.any():
                sim = adaptive_ref.simulate(lambda c: scan(c, integ), (h, w), LOOP["pass_spp"], LOOP["max_samples"], LOOP["tol"],
                                            LOOP["quantile"], LOOP["min_batches"], mask=mine_scan)
                assert (res["samples_total"], res["passes"], res["stopped_converged"], res["active"]) == \
                    (sim["samples_total"], sim["passes"], sim["stopped_converged"], sim["active"]), tag
                want = adaptive_ref.compose(lambda c: scan(c, integ), sim["counts"]).astype(F)
                _same(got, _shard_expect(_ordered(want, w, h, order), mine), ("pt_accum_add_adaptive",) + tag)
            else:
                _same(got, _shard_expect(mean32(1), mine), ("pt_accum_add_adaptive",) + tag)   # untouched
            _seen(("adaptive",) + tag[:2] + tag[3:], got)


# ---------------------------------------------------------------- 7. the noise and variance maps
def _noise_case(st, w, h, integ, freeze):
    """(error map, variance map), scanline float32: passes of 1, 1 and 1 samples, with the checkerboard frozen before
    the third (adaptive_ref.AdaptiveRef, which is noise_ref.NoiseRef bit for bit while nothing is frozen)."""
    render = lambda c: _cam_mean(st, w, h, c, integ)
    ref = adaptive_ref.AdaptiveRef(0, shape=(h, w))
    counts = np.zeros((h, w), dtype=np.uint32)
    frozen = rays_accum_ref.checkerboard(w, h) if freeze else np.zeros((h, w), dtype=bool)
    for c in (1, 2, 3):
        counts[~frozen if c == 3 else np.ones((h, w), dtype=bool)] = c
        ref.update(c, counts, adaptive_ref.compose(render, counts))
    return ref.error_map(), denoise_guided_ref.variance_ref(ref, counts)


@on_placements
@on_shapes
@pytest.mark.parametrize("freeze", [False, True], ids=["all_active", "frozen"])
def test_noise_maps_device(st, freeze, shape, placement):
    w, h, order = shape
    L = _lib.lib()
    for integ, k, n in MODES[1:]:
        emap, var = st.ref(("noise", w, h, integ, freeze), lambda: _noise_case(st, w, h, integ, freeze))
        mine = _mine(w, h, k, n, order)
        with st.r.accumulator(_cam(w, h), w, h, BOUNCES, integ, SEED, 0, k, n, order) as acc, acc.noise() as est:
            for c in (1, 2, 3):
                if c == 3 and freeze:
                    acc.freeze(_checker(w, h, order))
                acc.add(1)
                est.update()
            b = Bands(placement)
            d_rel2, d_var = b.out(w * h * 4, 4), b.out(w * h * 4, 4)
            b.ready()
            _lib.check(L.pt_noise_map_device(est._h, C.byref(_lib.NoiseParams(0.05, 0.01)), C.c_void_p(d_rel2.ptr), None))
            est.variance_device(d_var.ptr)
            what = ("noise maps", freeze, shape, placement, integ, k, n)
            b.verify(what)
            got = d_rel2.read(F), d_var.read(F)
            _same(got[0], _shard_expect(_ordered(emap, w, h, order), mine), ("pt_noise_map_device",) + what)
            _same(got[1], _shard_expect(_ordered(var, w, h, order), mine), ("pt_noise_variance_device",) + what)
            _seen(("noise", freeze, shape, integ, k, n), np.concatenate(got))
    if w * h > 1:
        assert np.isfinite(emap).any() and (var > 0).any()


# ---------------------------------------------------------------- 8. the denoisers
def _denoise_case(st, w, h):
    """(img, feat, var, filtered, guided-filtered), scanline: the oracle's 2-spp mean, the composed features, the
    variance map of three passes, and the two restatements at 5 iterations (steps 1..16)."""
    img = _cam_mean(st, w, h, SPP, 0).astype(F)
    feat = _features(st, w, h, "camera")
    var = _noise_case(st, w, h, 0, False)[1]
    return img, feat, var, denoise_ref.denoise_ref(img, feat, iterations=5), \
        denoise_guided_ref.denoise_guided_ref(img, feat, var, iterations=5)


@on_poisons
@on_placements
@on_shapes
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("entry", ["pt_denoise_device", "pt_denoise_guided_device"])
def test_denoise_device(st, entry, kernel, shape, placement, poison):
    w, h, order = shape
    img, feat, var, want, want_guided = st.ref(("denoise", w, h), lambda: _denoise_case(st, w, h))
    guided = entry == "pt_denoise_guided_device"
    want = _ordered(want_guided if guided else want, w, h, order)
    direct, tiled_max = KERNELS[kernel]
    for in_place in (False, True):
        b = Bands(placement, poison)
        d_in = b.inp(_ordered(img, w, h, order), 4, in_place=in_place)
        d_feat = b.inp(_ordered(feat, w, h, order), 16)
        d_var = b.inp(_ordered(var, w, h, order), 4) if guided else None
        d_out = d_in if in_place else b.out(w * h * 12, 4)
        b.ready()
        with direct_gather(direct, tiled_max):
            if guided:
                st.r.denoise_guided_device(d_in.ptr, d_feat.ptr, d_var.ptr, d_out.ptr, w, h, iterations=5, pixel_order=order)
            else:
                st.r.denoise_device(d_in.ptr, d_feat.ptr, d_out.ptr, w, h, iterations=5, pixel_order=order)
        what = (entry, kernel, shape, placement, poison, "in place" if in_place else "")
        b.verify(what)
        got = d_out.read(F, (w * h, 3))
        _same(got, want, what)
        _seen((entry, shape), got)                          # (every kernel, in place or not: the same bytes)
    if w * h > 1:
        assert want.tobytes() != _ordered(img, w, h, order).tobytes()


# ---------------------------------------------------------------- 9. temporal pushes
# forth and back along the orbit in steps of 0.16 rad: at each shape below some pixels reproject into the band x0 = -1, some
# into y0 = -1, some onto the last column and the last row (TemporalRef's own stats; asserted in the test)
TEMPORAL_POSES, TEMPORAL_STEP = (0, -1, 1), 0.16


def _temporal_case(st, w, h):
    """Three frames along the orbit: [(pose, img, feat, out, var)], scanline; the frames are random colours over the
    features the oracle's trace composes at each pose, the results temporal_ref.TemporalRef's."""
    rng = np.random.default_rng(w * 100 + h)
    ref = temporal_ref.TemporalRef(w, h)
    frames, stats = [], []
    for i in TEMPORAL_POSES:
        pose = temporal_ref.orbit_pose(i, TEMPORAL_STEP)
        feat = _features(st, w, h, "view", pose)
        img = rng.uniform(0, 4, (h, w, 3)).astype(F)
        out, var = ref.push(img, feat, (pose[0], 1.0, 3.0, 0.0, w, h), pose[1])
        frames.append((pose, img, feat, out, var))
        stats.append(dict(ref.stats))
    return frames, stats


@on_poisons
@on_placements
@on_shapes
def test_temporal_push_device(st, shape, placement, poison):
    """Three pushes along temporal_ref.orbit_pose on three histories: d_var present, d_var null, and in place."""
    w, h, order = shape
    frames, stats = st.ref(("temporal", w, h), lambda: _temporal_case(st, w, h))
    if w * h > 1:               # taps at x0 = -1, y0 = -1 and in the last column and row occur
        for key in ("x0_minus1", "y0_minus1", "x0_last", "y0_last", "tap_outside", "fractional"):
            assert sum(s.get(key, 0) for s in stats) > 0, key
    with st.r.temporal(w, h, pixel_order=order) as with_var, st.r.temporal(w, h, pixel_order=order) as no_var, \
            st.r.temporal(w, h, pixel_order=order) as alias:
        for i, (pose, img, feat, out, var) in enumerate(frames):
            cam, view = _cam(w, h, pose[0]), _view(pose[1])
            want, want_var = _ordered(out, w, h, order), _ordered(var, w, h, order)
            for name, hist in (("d_var", with_var), ("null d_var", no_var), ("in place", alias)):
                b = Bands(placement, poison)
                d_in = b.inp(_ordered(img, w, h, order), 4, in_place=name == "in place")
                d_feat = b.inp(_ordered(feat, w, h, order), 16)
                d_out = d_in if name == "in place" else b.out(w * h * 12, 4)
                d_var = None if name == "null d_var" else b.out(w * h * 4, 4)
                b.ready()
                hist.push_device(d_in.ptr, d_feat.ptr, d_out.ptr, cam, view, 0, None if d_var is None else d_var.ptr)
                what = ("pt_temporal_push_device", name, i, shape, placement, poison)
                b.verify(what)
                _same(d_out.read(F, (w * h, 3)), want, what)
                if d_var is not None:
                    _same(d_var.read(F), want_var, what + ("var",))


# ---------------------------------------------------------------- 10. the output step
@on_poisons
@on_placements
@on_scan_shapes
def test_tonemap_device(st, shape, placement, poison):
    w, h, _ = shape

    def make():
        rgb = _cam_mean(st, w, h, SPP, 0).astype(F).copy()
        edge = np.array([0.0, -0.0, 1e-45, 1e-38, 3.4028235e38, np.inf, np.nan, -0.5, -1.0, 1.0, 0.25, 0.999], dtype=F)
        flat = rgb.reshape(-1)
        flat[-min(len(edge), flat.size):] = edge[:min(len(edge), flat.size)]       # edge values against the back guard
        with np.errstate(all="ignore"):
            codes = np.vectorize(pt.tonemap_u8)(rgb.astype(np.float64)).astype(np.int64)
        codes[rgb < 0] = 2 ** 31 - 1                    # pt.h: the device variant marks negatives for the host to redo
        return rgb, codes.astype(np.int32)
    rgb, codes = st.ref(("tonemap", w, h), make)
    b = Bands(placement, poison)
    d_rgb, d_codes = b.inp(rgb, 4), b.out(w * h * 12, 4)
    b.ready()
    _lib.check(_lib.lib().pt_tonemap_device(st.r._h, C.c_void_p(d_rgb.ptr), w, h, C.c_void_p(d_codes.ptr), None))
    what = ("pt_tonemap_device", shape, placement, poison)
    b.verify(what)
    _same(d_codes.read(np.int32, (h, w, 3)), codes, what)


# ---------------------------------------------------------------- 11. lightmap finishing
RADII = (0, 1, 16)
MASKS = ("half", "one", "column0", "corners")


@on_poisons
@on_placements
@on_scan_shapes
@pytest.mark.parametrize("radius", RADII)
def test_lightmap_dilate_device(st, radius, shape, placement, poison):
    w, h, _ = shape
    img = st.ref(("odd", w, h), lambda: lr.odd_image(w, h, 17 * w + h))
    masks = st.ref(("masks", w, h, radius), lambda: lr.masks(w, h, radius, 1000 * radius + w))
    for name in MASKS:
        want, want_src = st.ref(("dilate", w, h, radius, name), lambda: lr.dilate(img, masks[name], radius))
        for variant in ("d_src", "null d_src", "in place"):
            b = Bands(placement, poison)
            d_in = b.inp(img, 4, in_place=variant == "in place")
            d_cov = b.inp(masks[name], 1)
            d_out = d_in if variant == "in place" else b.out(w * h * 12, 4)
            d_src = b.out(w * h * 4, 4) if variant == "d_src" else None
            b.ready()
            st.r.lightmap_dilate_device(d_in.ptr, d_cov.ptr, d_out.ptr, w, h, radius, None if d_src is None else d_src.ptr)
            what = ("pt_lightmap_dilate_device", name, variant, radius, shape, placement, poison)
            b.verify(what)
            _same(d_out.read(F, (h, w, 3)), want, what)
            if d_src is not None:
                _same(d_src.read(np.int32, (h, w)), want_src, what + ("src",))


MAPS = [(1, 1), (3, 5), (16, 16)]      # (map_w, map_h)


def _cornell_chart(lo=0.1, hi=0.9):
    """lightmap_ref.cornell_chart of the box alone: cornell.obj is loaded first, so its triangles keep their ids in
    cornell_blob, whose own bounds the blob moves."""
    return lr.cornell_chart(load_scene("cornell").arrays(), lo, hi)


def _shade_case(st, w, h):
    """(features (w*h,), table (nt, 6), maps): the composed camera features with record 0 named a sphere (prim = num_tris)
    and record 1 the last triangle, whose table row -- the table's last, against the guard -- is charted onto the point
    (1, 1): its lookup clamps to the map's last texel, against that guard."""
    feat = _features(st, w, h, "camera").reshape(-1).copy()
    tris, uvs, _ = _cornell_chart()
    table = rays.chart_uv_table(st.nt, tris, uvs)
    table[st.nt - 1] = 1.0
    feat["prim"][0] = st.nt
    if feat.size > 1:
        feat["prim"][1] = st.nt - 1
        feat["position"][1] = (0.1, 0.2, 0.3)
        feat["albedo"][1] = (0.5, 0.25, 0.75)
    rng = np.random.RandomState(w)
    maps = [(rng.rand(mh, mw, 3) * 4).astype(F) for mw, mh in MAPS]
    return feat, table, maps


@on_poisons
@on_placements
@on_scan_shapes
def test_lightmap_shade_device(st, shape, placement, poison):
    w, h, _ = shape
    feat, table, maps = st.ref(("shade", w, h), lambda: _shade_case(st, w, h))
    classes = set()
    for j, lm in enumerate(maps):
        fill, flags = ((0.25, -2.0, 7.5), lr.NO_ALBEDO) if j == 1 else ((0.0, 0.0, 0.0), 0)
        want, cls = st.ref(("shaded", w, h, j), lambda: lr.shade(feat, table, lm, st.arrays, fill, flags))
        classes |= set(np.unique(cls).tolist())
        if feat.size > 1:
            assert cls[0] == lr.SPHERE and cls[1] == lr.SHADED
            last = lm[-1, -1] if flags else (feat["albedo"][1] * lm[-1, -1]).astype(F)
            assert want[1].tobytes() == last.tobytes()      # the last texel itself, through the table's last row
        b = Bands(placement, poison)
        d_feat, d_tab, d_map = b.inp(feat, 16), b.inp(table, 4), b.inp(lm, 4)
        d_out = b.out(w * h * 12, 4)
        b.ready()
        st.r.lightmap_shade_device(d_feat.ptr, w * h, d_tab.ptr, d_map.ptr, lm.shape[1], lm.shape[0], d_out.ptr, fill, flags)
        what = ("pt_lightmap_shade_device", MAPS[j], shape, placement, poison)
        b.verify(what)
        _same(d_out.read(F, (w * h, 3)), want, what)
    if w * h > 1:
        assert {lr.SPHERE, lr.SHADED, lr.MISS} <= classes


# ---------------------------------------------------------------- 12. the context's scratch: small after large
def _scratch_ops(st_arrays):
    """name -> op(r, w, h, v): the bytes an entry point returns on renderer r at w x h with data set v (0 or 1: another
    seed, camera pose, mask, image)."""
    F6 = lambda a, b: np.concatenate([a, b], axis=1).astype(F)
    dev = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy()).cuda()
    host = lambda t, dtype: np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype)
    new = lambda nbytes: torch.full((nbytes,), gb.OUT_FILL, dtype=torch.uint8, device="cuda")
    pose = lambda v: temporal_ref.orbit_pose(5 * v)
    seed = lambda v: SEED + 77 * v
    rng = lambda w, h, v: np.random.default_rng(1000 * v + w)

    def ray_rows(w, h, v):
        o, d = rays.ortho_rays(POS, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.8 - 0.5 * v, 1.8 - 0.5 * v, w, h)
        return F6(o, d)

    def point_rows(w, h, v):
        p, n = rays.grid_points((-0.9 + 0.3 * v, 0.0, -0.9), (0.0, 0.0, 1.8 - 0.4 * v), (1.8 - 0.4 * v, 0.0, 0.0), w, h, 1e-3)
        return F6(p, n)

    def render(r, w, h, v):
        out = new(w * h * 12)
        torch.cuda.synchronize()
        stats = r.render_device(_cam(w, h, pose(v)[0]), out.data_ptr(), w, h, SPP, BOUNCES, v, seed(v), view=_view(pose(v)[1]))
        assert stats["split_pixels"] > 0                    # (an image this small is split into sample chunks: lbuf, pmemo)
        img, _ = r.render(_cam(w, h, pose(v)[0]), w, h, SPP, BOUNCES, v, seed(v), view=_view(pose(v)[1]))
        return host(out, F).tobytes() + img.tobytes()

    def render_async(r, w, h, v):
        outs = [new(w * h * 12), new(w * h * 12)]
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            r.render_device_async(_cam(w, h, pose(v)[0]), o.data_ptr(), w, h, SPP, BOUNCES, j, seed(v), view=_view(pose(v)[1]))
        r.wait(), r.wait()
        torch.cuda.synchronize()
        return host(outs[0], F).tobytes() + host(outs[1], F).tobytes()

    def features(r, w, h, v):
        out = new(w * h * 48)
        torch.cuda.synchronize()
        r.features_device(_cam(w, h, pose(v)[0]), out.data_ptr(), w, h, view=_view(pose(v)[1]))
        return host(out, np.uint8).tobytes()

    def render_rays(r, w, h, v):
        rows, out, feat = ray_rows(w, h, v), new(w * h * 12), new(w * h * 48)
        d = dev(rows)
        torch.cuda.synchronize()
        r.render_rays_device(d.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, v, seed(v))
        r.features_rays_device(d.data_ptr(), feat.data_ptr(), w, h)
        return host(out, F).tobytes() + host(feat, np.uint8).tobytes() + \
            r.render_rays(rows[:, :3], rows[:, 3:], w, h, SPP, BOUNCES, v, seed(v))[0].tobytes() + \
            r.features_rays(rows[:, :3], rows[:, 3:], w, h).tobytes() + \
            repr(sorted(r.classify_rays_device(d.data_ptr(), w * h).items())).encode()

    def render_irradiance(r, w, h, v):
        rows, out = point_rows(w, h, v), new(w * h * 12)
        d = dev(rows)
        torch.cuda.synchronize()
        r.render_irradiance_device(d.data_ptr(), out.data_ptr(), w, h, SPP, BOUNCES, v, seed(v))
        return host(out, F).tobytes() + r.render_irradiance(rows[:, :3], rows[:, 3:], w, h, SPP, BOUNCES, v, seed(v))[0].tobytes() + \
            repr(sorted(r.classify_points_device(d.data_ptr(), w * h).items())).encode()

    def queries(r, w, h, v):
        sets = raysets.ray_sets(st_arrays, w * h, 40 + v)
        o, d = sets["interior" if v == 0 else "outside"]
        rows, m = F6(o, d), w * h
        dr, tri, t, occ = dev(rows), new(m * 4), new(m * 4), new(m)
        tm = np.full(m, 0.5 + v, dtype=F)
        dtm = dev(tm)
        torch.cuda.synchronize()
        r.trace_device(dr.data_ptr(), m, tri.data_ptr(), t.data_ptr())
        r.occluded_device(dr.data_ptr(), m, occ.data_ptr(), dtm.data_ptr())
        return host(tri, np.int32).tobytes() + host(t, F).tobytes() + host(occ, np.uint8).tobytes() + \
            r.occluded(o, d, tm).tobytes() + b"".join(a.tobytes() for a in r.trace(o, d))

    def accumulators(r, w, h, v):
        rows, prow, res = ray_rows(w, h, v), point_rows(w, h, v), b""
        mask = rays_accum_ref.checkerboard(w, h, 1 + v)
        makers = (lambda: r.accumulator(_cam(w, h, pose(v)[0]), w, h, BOUNCES, v, seed(v), view=_view(pose(v)[1])),
                  lambda: r.accumulator_rays_device(dev(rows).data_ptr(), w, h, BOUNCES, v, seed(v)),
                  lambda: r.accumulator_points_device(dev(prow).data_ptr(), w, h, BOUNCES, v, seed(v)))
        for make in makers:
            out = new(w * h * 12)
            torch.cuda.synchronize()
            with make() as acc:
                acc.add(1, d_out_ptr=out.data_ptr())
                acc.freeze(mask)
                acc.add(1, d_out_ptr=out.data_ptr())
                res += host(out, F).tobytes() + acc.mean64().tobytes() + acc.active_pixels().tobytes()
            with make() as acc:
                info = acc.add_adaptive(1, 3, 0.5, 0.95, 2, d_out_ptr=out.data_ptr())
                emap, var = new(w * h * 4), new(w * h * 4)
                torch.cuda.synchronize()
                _lib.check(_lib.lib().pt_noise_map_device(acc._noise._h, C.byref(_lib.NoiseParams(0.05, 0.01)),
                                                          C.c_void_p(emap.data_ptr()), None))
                acc._noise.variance_device(var.data_ptr())
                res += host(out, F).tobytes() + host(emap, F).tobytes() + host(var, F).tobytes() + acc.counts().tobytes() + \
                    repr((info["passes"], info["samples_total"], info["active"])).encode()
            with make() as acc:
                acc.add_until(1, 3, 0.5, 0.95, 2, d_out_ptr=out.data_ptr())
                res += host(out, F).tobytes() + acc.mean64().tobytes()
        return res

    def session(r, w, h, v, tmp):
        path = str(tmp / ("s_%d_%d_%d.ptsession" % (w, h, v)))
        with r.accumulator(_cam(w, h, pose(v)[0]), w, h, BOUNCES, v, seed(v)) as acc:
            est = acc.noise()
            acc.add(1)
            est.update()
            acc.freeze(rays_accum_ref.checkerboard(w, h, 1 + v))
            acc.add(1)
            est.update()
            acc.save_session(path, est)
            want = acc.mean64().tobytes() + acc.counts().tobytes()
        acc, est = r.load_session(path)
        with acc:
            assert acc.mean64().tobytes() + acc.counts().tobytes() == want
            acc.add(1)
            est.update()
            return acc.mean64().tobytes() + est.error_map().tobytes() + open(path, "rb").read()

    def denoisers(r, w, h, v):
        g = rng(w, h, v)
        img = g.uniform(0, 4, (h, w, 3)).astype(F)
        feat = r.features(_cam(w, h, pose(v)[0]), w, h, view=_view(pose(v)[1]))
        var = g.uniform(0, 0.1, (h, w)).astype(F)
        d_img, d_feat, d_var, out, out2 = dev(img), dev(feat), dev(var), new(w * h * 12), new(w * h * 12)
        torch.cuda.synchronize()
        res = b""
        for kernel in sorted(KERNELS):
            with direct_gather(*KERNELS[kernel]):
                r.denoise_device(d_img.data_ptr(), d_feat.data_ptr(), out.data_ptr(), w, h, iterations=5)
                r.denoise_guided_device(d_img.data_ptr(), d_feat.data_ptr(), d_var.data_ptr(), out2.data_ptr(), w, h, iterations=5)
            res += host(out, F).tobytes() + host(out2, F).tobytes()
        return res

    def temporal(r, w, h, v):
        g = rng(w, h, v)
        res = b""
        with r.temporal(w, h) as t:
            for i in range(3):
                ps = temporal_ref.orbit_pose(i + 4 * v)
                cam, view = _cam(w, h, ps[0]), _view(ps[1])
                d_img, d_feat = dev(g.uniform(0, 4, (h, w, 3)).astype(F)), dev(r.features(cam, w, h, view=view))
                out, var = new(w * h * 12), new(w * h * 4)
                torch.cuda.synchronize()
                t.push_device(d_img.data_ptr(), d_feat.data_ptr(), out.data_ptr(), cam, view, 0, var.data_ptr())
                res += host(out, F).tobytes() + host(var, F).tobytes()
            return res + t.history_length().tobytes()

    def tonemap(r, w, h, v):
        d_rgb, out = dev(rng(w, h, v).uniform(-0.5, 2, (h, w, 3)).astype(F)), new(w * h * 12)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().pt_tonemap_device(r._h, C.c_void_p(d_rgb.data_ptr()), w, h, C.c_void_p(out.data_ptr()), None))
        return host(out, np.int32).tobytes()

    def lightmap(r, w, h, v):
        img, mask = lr.odd_image(w, h, 3 + v), lr.masks(w, h, 16, 9 + v)["sparse" if v else "half"]
        d_img, d_cov, out, src, shaded = dev(img), dev(mask), new(w * h * 12), new(w * h * 4), new(w * h * 12)
        feat = r.features(_cam(w, h, pose(v)[0]), w, h, view=_view(pose(v)[1]))
        tris, uvs, _ = _cornell_chart(0.1 + 0.1 * v, 0.9)
        d_feat, d_tab = dev(feat), dev(rays.chart_uv_table(st_arrays["tris"].shape[0], tris, uvs))
        d_map = dev(rng(w, h, v).uniform(0, 4, (5 + v, 3 + v, 3)).astype(F))
        torch.cuda.synchronize()
        r.lightmap_dilate_device(d_img.data_ptr(), d_cov.data_ptr(), out.data_ptr(), w, h, 16, src.data_ptr())
        r.lightmap_shade_device(d_feat.data_ptr(), w * h, d_tab.data_ptr(), d_map.data_ptr(), 3 + v, 5 + v, shaded.data_ptr())
        return host(out, F).tobytes() + host(src, np.int32).tobytes() + host(shaded, F).tobytes()

    return dict(render=render, render_async=render_async, features=features, render_rays=render_rays,
                render_irradiance=render_irradiance, queries=queries, accumulators=accumulators, session=session,
                denoisers=denoisers, temporal=temporal, tonemap=tonemap, lightmap=lightmap)


SCRATCH_OPS = ["render", "render_async", "features", "render_rays", "render_irradiance", "queries", "accumulators", "session",
               "denoisers", "temporal", "tonemap", "lightmap"]


@pytest.mark.parametrize("op", SCRATCH_OPS)
def test_scratch_small_after_large(st, op, tmp_path):
    """The context keeps grow-on-demand scratch, so a kernel that read a stale element of it instead of an out-of-image
    default would give results that depend on earlier calls.  On the shared renderer every group of entry points runs
    at 65 x 33 with one data set, at 37 x 19 with another (seed, integrator, camera pose, rays, points, mask, image),
    and at 65 x 33 again: the middle result equals, in every bit, the same calls on a freshly created renderer, and
    the outer two equal each other.  Which scratch each group reaches:

      render, render_async   rb[0] and rb[1]: spill, pix_states, and lbuf and pmemo (images this small are split into
                             sample chunks: stats split_pixels > 0); the host render also scratch_out
      features               rb[0].spill
      render_rays            rb[].spill, pix_states; the host variants rays_stage and scratch_out
      render_irradiance      rb[].spill, pix_states; the host variant rays_stage and scratch_out
      queries                rb[0].spill; pt_occluded (host) query_stage
      accumulators           rb[].spill, pix_states through every pass of pt_accum_add, _add_until and _add_adaptive,
                             with the noise maps read afterwards (the estimator's planes are the accumulator's own)
      session                session (staging of pt_session_save / _load), then a pass on what was loaded
      denoisers              denoise (the ping-pong planes of pt_denoise_device and pt_denoise_guided_device)
      temporal, tonemap, lightmap   none of the context's scratch: they must not depend on it either"""
    fn = _scratch_ops(st.arrays)[op]
    run = (lambda r, w, h, v: fn(r, w, h, v, tmp_path)) if op == "session" else fn
    big = run(st.r, 65, 33, 0)
    small = run(st.r, 37, 19, 1)
    again = run(st.r, 65, 33, 0)
    with pt.Renderer(st.scene, 0) as fresh:
        want = run(fresh, 37, 19, 1)
    assert len(small) == len(want) and len(big) == len(again)
    assert small == want, "%s: 37 x 19 after 65 x 33 differs from a fresh renderer's" % op
    assert big == again, "%s: 65 x 33 differs after a 37 x 19 call" % op
    assert big[:len(small)] != small
