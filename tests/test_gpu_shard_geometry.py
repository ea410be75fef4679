"""Shard geometry on every GPU path: tiles larger than 8x8 on images they do not divide (several 8x8 blocks per tile,
most of an edge tile's slots outside the image), uneven shards, and shards that own no tile at all (shard_index >=
the tile count: an 8-GPU job on a small preview image).  The plain render, the accumulator and its checkpoint file,
the noise estimator, adaptive sampling with its device-built active list, and the feature buffers are each run on the
geometries of tests/shard_geometries.py and compared bit for bit with the references the suite already trusts: the
oracle's f64 image, tests/noise_ref.py, tests/adaptive_ref.py, the host composition of the features, and
shard.shard_pixels for which pixels a shard owns and in what order.  cornell_blob, bounces 3, seed 1234, at most 9
samples per pixel (the adaptive loop's own case, adaptive_ref.LOOP, apart)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, scenes, shard

import adaptive_ref
import denoise_guided_ref
import denoise_ref
import noise_ref
from adaptive_ref import LOOP
from shard_geometries import GEOMETRIES, Geometry
from test_gpu_adaptive import Sched

pytestmark = pytest.mark.gpu

CAM = scenes.CORNELL_CAMERA              # pos (0, 1, 3), film 1, focal 3, radius 0: kernel.cu:642-648
BOUNCES, SEED, SPP = 3, 1234, 5
TOLS = (0.05, 0.25, 1.0)
HEADER_BYTES, RECORD_BYTES = 128, 48
SHARD_INDEX_AT = 16 + 32                 # checkpoint header: pt_params at 16, its shard_index at +32
SENTINEL = 0xA5                          # every byte of a device buffer before the call under test
G = {gid: Geometry(gid) for gid in GEOMETRIES}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _cam(g):
    return pt.make_camera(width=g.w, height=g.h, **CAM)


def _kw(g, k):
    """The shard arguments of Renderer.accumulator / features for shard k of geometry g."""
    return dict(shard_index=k, shard_count=g.shards, pixel_order=g.order, tile=(g.tw, g.th))


def _shard(g, k):
    """(order, mine): the scanline ids of shard k's pixels in work order, and the shard's mask, shape (H, W)."""
    order = shard.shard_pixels(g.w, g.h, k, g.shards, g.tw, g.th)
    assert len(order) == g.pixels[k], (g, k)
    mine = np.zeros(g.w * g.h, dtype=bool)
    mine[order] = True
    return order, mine.reshape(g.h, g.w)


def _index(g):
    yy, xx = np.mgrid[0:g.h, 0:g.w]
    return shard.morton_index(xx, yy).astype(np.int64)


def _scan(g, a):
    """An array in the geometry's pixel order as a scanline (H, W, ...) array."""
    a = np.asarray(a)
    if not g.order:
        return a
    return a.reshape((g.w * g.h,) + a.shape[1:])[_index(g)]


def _ordered(g, a):
    """A scanline (H, W) array in the geometry's pixel order."""
    a = np.asarray(a)
    if not g.order:
        return a
    out = np.zeros(g.w * g.h, dtype=a.dtype)
    out[_index(g).reshape(-1)] = a.reshape(-1)
    return out


@pytest.fixture(scope="module")
def cb():
    s = load_scene("cornell_blob")
    with pt.Renderer(s, 0) as r:
        yield s, r


_ORACLE = {}


def _oracle(scene, g, n, integ):
    """(f64 image, counters) of the oracle after n samples of every pixel of g's image, once per configuration."""
    k = (g.w, g.h, n, integ)
    if k not in _ORACLE:
        import oracle
        if "scene" not in _ORACLE:
            _ORACLE["scene"] = oracle.OracleScene(scene.arrays())
        ocam = oracle.camera(CAM["pos"], CAM["dist_from_film"], CAM["focal_length"], CAM["radius"], g.w, g.h)
        _ORACLE[k] = oracle.render(_ORACLE["scene"], ocam, g.w, g.h, n, BOUNCES, integ, SEED)
    return _ORACLE[k]


def _image(scene, g, integ):
    return lambda n: _oracle(scene, g, n, integ)[0]


def _sentinel(nbytes):
    import torch
    buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def _host(buf, dtype, shape):
    return np.frombuffer(buf.cpu().numpy().tobytes(), dtype=dtype).reshape(shape)


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


def _accumulator(r, g, k, integ=0):
    return r.accumulator(_cam(g), g.w, g.h, bounces=BOUNCES, integrator=integ, seed=SEED, **_kw(g, k))


# ---------------------------------------------------------------- 1. the plain render
def _plain(cb, g, integ, flags=0):
    s, r = cb
    ref, cnt = _oracle(s, g, SPP, integ)
    ref32 = ref.astype(np.float32)
    total = np.zeros((g.h, g.w, 3), dtype=np.float32)
    rays = 0
    for k in range(g.shards):
        order, mine = _shard(g, k)
        img, st = r.render(_cam(g), g.w, g.h, SPP, bounces=BOUNCES, integrator=integ, seed=SEED, flags=flags, shard_index=k,
                           shard_count=g.shards, pixel_order=g.order, tile_w=g.tw, tile_h=g.th)
        img = _scan(g, img)
        assert _bits(img[~mine]) == bytes(12 * int((~mine).sum())), (g, k)          # exactly 0 outside the shard
        assert _bits(img[mine]) == _bits(ref32[mine]), (g, k)
        assert st["samples"] == len(order) * SPP, (g, k)
        assert st["rays_nominal"] == len(order) * SPP * (BOUNCES + 1), (g, k)
        assert math.isfinite(st["seconds"]) and st["seconds"] >= 0.0
        if flags & pt.PT_FLAG_COUNT and len(order):
            assert st["node_tests"] > 0 and st["tri_tests"] > 0
        total += img
        rays += st["rays_reference"]
    assert _bits(total) == _bits(ref32), g
    assert rays == cnt["traces"], g


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid", sorted(GEOMETRIES))
def test_plain_render(cb, gid, integ):
    _plain(cb, G[gid], integ)


@pytest.mark.parametrize("flags", [pt.PT_FLAG_REFERENCE_TRAVERSAL, pt.PT_FLAG_COUNT], ids=["tile_kernel", "count"])
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid", ["A", "C"])
def test_plain_render_on_the_other_kernels(cb, gid, integ, flags):
    """PT_FLAG_REFERENCE_TRAVERSAL takes the tile kernel (one wave per 8x8 block of a tile), PT_FLAG_COUNT the
    counting instances of the wavefront kernels."""
    _plain(cb, G[gid], integ, flags)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid", ["A", "B"])
def test_render_device_writes_the_shards_pixels_only(cb, gid, integ):
    s, r = cb
    g = G[gid]
    ref32 = _oracle(s, g, SPP, integ)[0].astype(np.float32)
    for k in range(g.shards):
        order, mine = _shard(g, k)
        buf = _sentinel(g.w * g.h * 12)
        st = r.render_device(_cam(g), buf.data_ptr(), g.w, g.h, SPP, bounces=BOUNCES, integrator=integ, seed=SEED,
                             shard_index=k, shard_count=g.shards, tile_w=g.tw, tile_h=g.th)
        got = _host(buf, np.float32, (g.h, g.w, 3))
        assert st["samples"] == len(order) * SPP
        assert _untouched(got[~mine]), (g, k)
        assert _bits(got[mine]) == _bits(ref32[mine]), (g, k)
        if not len(order):
            assert _untouched(got)


# ---------------------------------------------------------------- 2. the accumulator
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid", ["A", "B", "C", "E", "F"])
def test_accumulator(cb, gid, integ):
    s, r = cb
    g = G[gid]
    for k in range(g.shards):
        order, mine = _shard(g, k)
        with _accumulator(r, g, k, integ) as acc:
            for n in (2, 3):
                st = acc.add(n)
                assert st["samples"] == len(order) * n, (g, k)
                want = np.where(mine[..., None], _oracle(s, g, acc.samples, integ)[0], 0.0)
                assert _bits(_scan(g, acc.mean64())) == _bits(want), (g, k, acc.samples)
                assert _bits(_scan(g, acc.image())) == _bits(want.astype(np.float32)), (g, k, acc.samples)
                assert _bits(_scan(g, acc.counts())) == _bits(np.where(mine, acc.samples, 0).astype(np.uint32)), (g, k)
            assert acc.samples == 5


def _records(path, g):
    with open(path, "rb") as fh:
        raw = fh.read()
    assert len(raw) == HEADER_BYTES + g.w * g.h * RECORD_BYTES
    rec = np.frombuffer(raw[HEADER_BYTES:], dtype=np.dtype([("rng", "<u4", (6,)), ("mean", "<f8", (3,))]))
    return raw, rec.reshape(g.h, g.w)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid,k", [("A", 1), ("B", 4)], ids=["A1", "B4_empty"])
def test_checkpoint(cb, tmp_path, gid, k, integ):
    s, r = cb
    g = G[gid]
    order, mine = _shard(g, k)
    f5, f9, f9_resumed = (str(tmp_path / n) for n in ("at5.ptacc", "at9.ptacc", "at9_resumed.ptacc"))
    with _accumulator(r, g, k, integ) as acc:
        acc.add(2)
        acc.add(3)
        acc.save(f5)
        acc.add(4)                                          # the run that was never saved and loaded
        acc.save(f9)
        straight = acc.mean64()
    info = pt.accum_file_info(f5)
    p = info["params"]
    assert (p.width, p.height, p.tile_w, p.tile_h) == (g.w, g.h, g.tw, g.th)
    assert (p.shard_index, p.shard_count, p.pixel_order, p.integrator, p.bounces, p.seed, p.spp) == \
        (k, g.shards, g.order, integ, BOUNCES, SEED, 0)
    assert info["samples"] == 5
    raw, rec = _records(f5, g)
    assert _bits(rec[~mine]) == bytes(RECORD_BYTES * int((~mine).sum()))            # outside the shard: all zero
    assert _bits(rec["mean"][mine]) == _bits(_oracle(s, g, 5, integ)[0][mine])
    if not len(order):
        assert raw[HEADER_BYTES:] == bytes(g.w * g.h * RECORD_BYTES)                # a header plus all-zero records
    else:
        assert rec["rng"][mine].any(axis=1).all()                                   # every pixel of the shard has a stream
    with r.load_accumulator(f5) as acc:
        # the header carries the shard: the loaded accumulator is this shard of this grid and no other
        q = acc.params
        assert (q.shard_index, q.shard_count, q.tile_w, q.tile_h) == (k, g.shards, g.tw, g.th)
        assert acc.samples == 5 and acc.active_pixels().size == len(order)
        assert _bits(acc.active_pixels()) == _bits(order)
        assert _bits(acc.mean64()[mine]) == _bits(_oracle(s, g, 5, integ)[0][mine]) and not acc.mean64()[~mine].any()
        st = acc.add(4)
        assert st["samples"] == len(order) * 4 and acc.samples == 9
        assert _bits(acc.mean64()) == _bits(straight)
        assert _bits(acc.mean64()) == _bits(np.where(mine[..., None], _oracle(s, g, 9, integ)[0], 0.0))
        acc.save(f9_resumed)
    with open(f9, "rb") as a, open(f9_resumed, "rb") as b:                          # the streams too, byte for byte
        assert a.read() == b.read()
    if not len(order):
        # the records say nothing about the shard, the header alone does: the same records under shard 0's header are
        # shard 0's accumulator (at 5 samples, every mean still the file's 0), not the empty shard's
        other = str(tmp_path / "as_shard0.ptacc")
        with open(other, "wb") as fh:
            fh.write(raw[:SHARD_INDEX_AT] + np.int32(0).tobytes() + raw[SHARD_INDEX_AT + 4:])
        assert pt.accum_file_info(other)["params"].shard_index == 0
        with r.load_accumulator(other) as acc:
            assert acc.params.shard_index == 0 and acc.samples == 5
            assert _bits(acc.active_pixels()) == _bits(_shard(g, 0)[0]) and not acc.mean64().any()


# ---------------------------------------------------------------- 3. the noise estimator
def _noise_params(tol=0.05, y_floor=0.01):
    return _lib.NoiseParams(tol, y_floor)


def _check_estimator(g, k, acc, est, ref, counts):
    """State, summary, error map and variance map of `est` against the restatement `ref` (fed with the oracle's
    images) restricted to the shard; the device variants leave a sentinel outside it."""
    order, mine = _shard(g, k)
    for tol in TOLS:
        got = est.update(tol=tol)                           # (folds at most once: the later calls re-summarise)
        want = ref.summary(tol, noise_ref.Y_FLOOR, mine)
        assert got["samples"] == acc.samples and got["pixels"] == len(order) == want["pixels"], (g, k)
        assert {key: got[key] for key in want} == want, (g, k, tol)
        assert len(got["hist"]) == 64 and sum(got["hist"]) == len(order)
    mu, m2 = est.read()
    assert _bits(mu) == _bits(np.where(mine, ref.mu, 0.0)) and _bits(m2) == _bits(np.where(mine, ref.m2, 0.0)), (g, k)
    emap, var = ref.error_map(), denoise_guided_ref.variance_ref(ref, counts)
    zero = np.float32(0.0)
    assert _bits(est.error_map()) == _bits(np.where(mine, emap, zero)), (g, k)
    assert _bits(est.variance()) == _bits(np.where(mine, var, zero)), (g, k)
    buf = _sentinel(g.w * g.h * 4)
    _lib.check(_lib.lib().pt_noise_map_device(est._h, C.byref(_noise_params()), C.c_void_p(buf.data_ptr()), None))
    dev = _host(buf, np.float32, (g.h, g.w))
    assert _untouched(dev[~mine]) and _bits(dev[mine]) == _bits(emap[mine]), (g, k)
    buf = _sentinel(g.w * g.h * 4)
    est.variance_device(buf.data_ptr())
    dev = _host(buf, np.float32, (g.h, g.w))
    assert _untouched(dev[~mine]) and _bits(dev[mine]) == _bits(var[mine]), (g, k)
    if not len(order):
        assert _untouched(dev)


@pytest.mark.parametrize("gid", ["A", "C", "E"])
def test_noise_estimator(cb, gid):
    s, r = cb
    g = G[gid]
    render = _image(s, g, 0)
    seen = 0
    for k in range(g.shards):
        order, mine = _shard(g, k)
        with _accumulator(r, g, k) as acc, acc.noise() as est:
            ref = noise_ref.NoiseRef(0, shape=(g.h, g.w))
            for n in (2, 3, 4):
                acc.add(n)
                assert ref.update(acc.samples, render(acc.samples))
                _check_estimator(g, k, acc, est, ref, acc.samples)
            last = est.update(tol=0.25)
            assert last["batches"] == 3 and last["samples"] == 9
            seen += last["converged"]
    assert 0 < seen < g.w * g.h                            # not trivially all or nothing


@pytest.mark.parametrize("gid", ["A", "C", "E"])
def test_noise_estimator_after_a_freeze(cb, gid):
    """A host freeze before the last pass: the estimator goes to its per-pixel W_q / b_q planes, strided by slots."""
    s, r = cb
    g = G[gid]
    render = _image(s, g, 0)
    checker = (np.add.outer(np.arange(g.h), np.arange(g.w)) % 2) == 0
    for k in g.nonempty():
        order, mine = _shard(g, k)
        with _accumulator(r, g, k) as acc, acc.noise() as est:
            ref = adaptive_ref.AdaptiveRef(0, shape=(g.h, g.w))
            counts = np.zeros((g.h, g.w), dtype=np.uint32)
            frozen = ~mine
            for n in (2, 3, 4):
                if n == 4:
                    acc.freeze(checker)
                    frozen = frozen | checker
                st = acc.add(n)
                assert st["samples"] == int((~frozen).sum()) * n, (g, k)
                counts[~frozen] = acc.samples
                assert _bits(acc.counts()) == _bits(counts)
                assert ref.update(acc.samples, counts, adaptive_ref.compose(render, counts))
                _check_estimator(g, k, acc, est, ref, counts)
            assert sorted(np.unique(ref.bq[mine])) == [2, 3] and sorted(np.unique(ref.Wq[mine])) == [5, 9]
            # the device freeze: what the restatement calls converged among the active pixels of the shard
            want = ref.converged(0.25) & ~frozen
            newly, active = est.freeze(tol=0.25)
            assert (newly, active) == (int(want.sum()), int((~(frozen | want)).sum())), (g, k)
            frozen = frozen | want
            assert _bits(acc.active_pixels()) == _bits(order[~frozen.reshape(-1)[order]])


# ---------------------------------------------------------------- 4. adaptive sampling
class _Scanline:
    """An accumulator seen in scanline order whatever its pixel order: what Sched compares its expectations with."""

    def __init__(self, acc, g):
        self._acc, self._g = acc, g

    @property
    def samples(self):
        return self._acc.samples

    def add(self, k, **kw):
        return self._acc.add(k, **kw)

    def freeze(self, mask):
        self._acc.freeze(_ordered(self._g, np.asarray(mask, dtype=bool)))

    def counts(self):
        return _scan(self._g, self._acc.counts())

    def mean64(self):
        return _scan(self._g, self._acc.mean64())

    def image(self):
        return _scan(self._g, self._acc.image())

    def active_pixels(self):
        return self._acc.active_pixels()


def _schedule(sc, g, render=None):
    """add 2, freeze a checkerboard, add 3, freeze the left half, add 4; counts and the active list after every step."""
    checker = (np.add.outer(np.arange(g.h), np.arange(g.w)) % 2) == 0
    left = np.zeros((g.h, g.w), dtype=bool)
    left[:, : g.w // 2] = True
    sc.check_counts_and_list()
    sc.add(2)
    sc.check_counts_and_list()
    sc.freeze(checker)
    sc.check_counts_and_list()
    sc.add(3)
    sc.check_counts_and_list()
    sc.freeze(left)
    sc.check_counts_and_list()
    sc.add(4)
    sc.check_counts_and_list()
    if render is not None:
        sc.check_image(render)


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("gid", ["A", "C", "D", "F"])
def test_adaptive_schedule(cb, gid, integ):
    s, r = cb
    g = G[gid]
    render = _image(s, g, integ)
    mean = np.zeros((g.h, g.w, 3), dtype=np.float64)
    counts = np.zeros((g.h, g.w), dtype=np.uint32)
    for k in g.nonempty():                                  # (the empty shards: test_empty_shard)
        order, mine = _shard(g, k)
        with _accumulator(r, g, k, integ) as acc:
            sc = Sched(_Scanline(acc, g), g.w, g.h, k, g.shards, tile=(g.tw, g.th))
            assert _bits(sc.order) == _bits(order) and (sc.mine == mine).all()
            _schedule(sc, g, render)
            assert not sc.acc.mean64()[~mine].any() and not sc.acc.counts()[~mine].any()
            mean += sc.acc.mean64()
            counts += sc.acc.counts()
    # the union over the shards is the unsharded accumulator driven by the same schedule
    with r.accumulator(_cam(g), g.w, g.h, bounces=BOUNCES, integrator=integ, seed=SEED, pixel_order=g.order) as acc:
        sc = Sched(_Scanline(acc, g), g.w, g.h)
        _schedule(sc, g)
        assert _bits(sc.acc.mean64()) == _bits(mean) and _bits(sc.acc.counts()) == _bits(counts)
    assert sorted(np.unique(counts)) == [2, 5, 9]
    assert _bits(mean) == _bits(adaptive_ref.compose(render, counts))


@pytest.mark.parametrize("integ", [0, 1])
def test_add_adaptive_on_a_shard(cb, integ):
    s, r = cb
    g = G["A"]
    order, mine = _shard(g, 0)
    render = _image(s, g, integ)
    with _accumulator(r, g, 0, integ) as acc:
        res = acc.add_adaptive(LOOP["pass_spp"], LOOP["cap"], tol=LOOP["tol"], quantile=LOOP["quantile"],
                               min_batches=LOOP["min_batches"])
        counts, mean, state, emap = acc.counts(), acc.mean64(), acc._noise.read(), acc._noise.error_map()
        active = acc.active_pixels()
    sim = adaptive_ref.simulate(render, (g.h, g.w), mask=mine, **LOOP)
    assert not sim["counts"][~mine].any() and 0 < sim["samples_total"] < len(order) * LOOP["cap"]
    assert _bits(counts) == _bits(sim["counts"]) and res["samples_total"] == sim["samples_total"]
    assert (res["passes"], res["stopped_converged"], res["active"]) == (sim["passes"], sim["stopped_converged"], sim["active"])
    assert res["summary"]["pixels"] == len(order)
    assert {key: res["summary"][key] for key in sim["summary"]} == sim["summary"]
    assert _bits(mean) == _bits(adaptive_ref.compose(render, counts))
    assert _bits(state[0]) == _bits(sim["est"].mu) and _bits(state[1]) == _bits(sim["est"].m2)
    assert _bits(emap) == _bits(np.where(mine, sim["est"].error_map(), np.float32(0.0)))
    assert active.size == res["active"] and set(active) <= set(order)


# ---------------------------------------------------------------- 5. the feature buffers
_FEATURES = {}


def _features_ref(cb, g):
    s, r = cb
    if (g.w, g.h) not in _FEATURES:
        _FEATURES[(g.w, g.h)] = denoise_ref.features_ref(s.arrays(), _cam(g), g.w, g.h, r.trace)
    return _FEATURES[(g.w, g.h)]


@pytest.mark.parametrize("gid", ["A", "C", "D", "F"])
def test_features(cb, gid):
    s, r = cb
    g = G[gid]
    ref = _features_ref(cb, g)
    assert (ref["prim"] >= 0).any()
    none = np.zeros(1, dtype=pt.FEATURE)
    none["prim"] = -1
    for k in range(g.shards):
        order, mine = _shard(g, k)
        host = _scan(g, r.features(_cam(g), g.w, g.h, **_kw(g, k)))
        assert _bits(host[mine]) == _bits(ref[mine]), (g, k)
        assert _bits(host[~mine]) == none.tobytes() * int((~mine).sum()), (g, k)
        buf = _sentinel(g.w * g.h * 48)
        r.features_device(_cam(g), buf.data_ptr(), g.w, g.h, **_kw(g, k))
        dev = _scan(g, _host(buf, pt.FEATURE, (g.w * g.h,) if g.order else (g.h, g.w)))
        assert _bits(dev[mine]) == _bits(ref[mine]), (g, k)
        assert _untouched(dev[~mine]), (g, k)
        if not len(order):
            assert _untouched(dev)


# ---------------------------------------------------------------- 6. empty shards
def _next_launch_is_clean(cb, g):
    """A non-empty shard on the same context, plain and accumulated, against the oracle: the empty launch before it
    left no counter and no cached state behind."""
    s, r = cb
    order, mine = _shard(g, 0)
    ref = _oracle(s, g, 2, 0)[0]
    img, st = r.render(_cam(g), g.w, g.h, 2, bounces=BOUNCES, seed=SEED, shard_index=0, shard_count=g.shards,
                       tile_w=g.tw, tile_h=g.th)
    assert _bits(img) == _bits(np.where(mine[..., None], ref, 0.0).astype(np.float32))
    assert st["samples"] == len(order) * 2 and st["rays_nominal"] == len(order) * 2 * (BOUNCES + 1)
    assert st["work_units"] >= len(order) and 0 < st["rays_traced"] <= st["rays_reference"]
    with _accumulator(r, g, 0) as acc:
        st = acc.add(2)
        assert st["samples"] == len(order) * 2
        assert _bits(acc.mean64()) == _bits(np.where(mine[..., None], ref, 0.0))


@pytest.mark.parametrize("gid,k", [("B", 4), ("E", 1)])
def test_empty_shard(cb, gid, k):
    """What include/pt/pt.h promises of a shard that owns no tile, call by call."""
    s, r = cb
    g = G[gid]
    order, mine = _shard(g, k)
    assert len(order) == 0 and k >= len(shard.shard_tiles(g.w, g.h, 0, 1, g.tw, g.th))
    zero_stats = ("samples", "rays_traced", "rays_reference", "rays_nominal", "work_units", "split_pixels")
    # pt_render
    for integ in (0, 1):
        img, st = r.render(_cam(g), g.w, g.h, SPP, bounces=BOUNCES, integrator=integ, seed=SEED, shard_index=k,
                           shard_count=g.shards, tile_w=g.tw, tile_h=g.th)
        assert _bits(img) == bytes(g.w * g.h * 12)
        assert [st[key] for key in zero_stats] == [0] * len(zero_stats), st
        assert math.isfinite(st["seconds"]) and math.isfinite(st["kernel_ms"])
        _next_launch_is_clean(cb, g)
    # pt_accum_add, _read, _counts
    with _accumulator(r, g, k) as acc:
        buf = _sentinel(g.w * g.h * 12)
        for n, total in ((2, 2), (3, 5)):
            st = acc.add(n, d_out_ptr=buf.data_ptr())
            assert [st[key] for key in zero_stats] == [0] * len(zero_stats), st
            assert acc.samples == total                    # nothing is frozen: the count advances
        assert _untouched(_host(buf, np.float32, (g.h, g.w, 3)))
        assert not acc.image().any() and not acc.mean64().any() and not acc.counts().any()
        _next_launch_is_clean(cb, g)
        # pt_accum_freeze with an all-ones mask, pt_accum_active
        acc.freeze(np.ones((g.h, g.w), dtype=bool))
        assert acc.active_pixels().size == 0
        assert acc.add(2)["samples"] == 0 and acc.samples == 7   # (the freeze froze nothing: still the plain path)
        _next_launch_is_clean(cb, g)
    # pt_noise_update, pt_noise_freeze, the maps
    with _accumulator(r, g, k) as acc, acc.noise() as est:
        first = est.update()
        assert (first["samples"], first["batches"], first["pixels"], first["converged"]) == (0, 0, 0, 0)
        for i, n in enumerate((2, 3, 4)):
            acc.add(n)
            got = est.update(tol=1.0)
            assert (got["samples"], got["batches"]) == (acc.samples, i + 1)
            assert got["pixels"] == 0 and got["converged"] == 0 and got["hist"] == [0] * 64
        assert est.update()["batches"] == 3                # no new samples: nothing folded
        assert est.freeze(tol=1.0) == (0, 0)
        assert not any(a.any() for a in est.read()) and not est.error_map().any() and not est.variance().any()
        assert acc.active_pixels().size == 0
        _next_launch_is_clean(cb, g)
    # pt_accum_add_until: 0 >= ceil(q * 0), so it stops as soon as min_batches passes are folded
    with _accumulator(r, g, k) as acc:
        res = acc.add_until(2, 9, tol=0.05, quantile=0.95, min_batches=3)
        assert res["passes"] == 3 and res["stopped_converged"] is True and res["samples"] == acc.samples == 6
        assert (res["summary"]["batches"], res["summary"]["pixels"], res["summary"]["converged"]) == (3, 0, 0)
        _next_launch_is_clean(cb, g)
    # pt_accum_add_adaptive: no pixel is active, so no pass runs
    with _accumulator(r, g, k) as acc:
        acc.add(2)
        res = acc.add_adaptive(2, 9, tol=0.05, quantile=0.95, min_batches=2)
        assert res["passes"] == 0 and res["stopped_converged"] is True
        assert res["active"] == 0 and res["samples_total"] == 0 and res["samples"] == acc.samples == 2
        assert res["summary"]["pixels"] == 0 and res["summary"]["hist"] == [0] * 64
        _next_launch_is_clean(cb, g)
    # pt_render_features
    none = np.zeros(1, dtype=pt.FEATURE)
    none["prim"] = -1
    assert _bits(r.features(_cam(g), g.w, g.h, **_kw(g, k))) == none.tobytes() * (g.w * g.h)
    _next_launch_is_clean(cb, g)
