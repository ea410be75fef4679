"""Ray queries on device buffers (pt_trace_device, pt_occluded_device, pt_occluded; kernel query_rays): every answer
against the CPU oracle -- oracle.trace_batch gives (tri, t), and occ = (tri >= 0) & (t < tmax) is evaluated in numpy
float32 (tests/query_cases.py) -- never against the library.  Device buffers are torch tensors with 64 sentinel
entries behind the n the call is given."""
import os

import numpy as np
import pytest
import torch

from conftest import golden, load_scene

import cudapathtracer_amd as pt
from cudapathtracer_amd import _lib, scenes

import query_cases as qc

pytestmark = pytest.mark.gpu

N = 5000
SEED = 31
PAD = 64
TRI_SENTINEL, T_SENTINEL, OCC_SENTINEL = -77, -7.0, 0xAB


def _dev(x):
    x = np.ascontiguousarray(x)
    if x.size == 0:   # (a valid pointer for n = 0 too)
        return torch.zeros(8, dtype=torch.from_numpy(x).dtype, device="cuda")
    return torch.from_numpy(x).cuda()


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32), len(o)


def trace_dev(r, o, d, reference_bvh=False, stream_ptr=None):
    """trace_device on fresh sentinel-filled buffers of n + PAD entries; asserts the tail untouched."""
    rays, n = _rays(o, d)
    dr = _dev(rays)
    tri = torch.full((n + PAD,), TRI_SENTINEL, dtype=torch.int32, device="cuda")
    t = torch.full((n + PAD,), T_SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.trace_device(dr.data_ptr(), n, tri.data_ptr(), t.data_ptr(), reference_bvh=reference_bvh, stream_ptr=stream_ptr)
    tri, t = tri.cpu().numpy(), t.cpu().numpy()
    assert (tri[n:] == TRI_SENTINEL).all() and (t[n:] == np.float32(T_SENTINEL)).all()
    return tri[:n], t[:n]


def occ_dev(r, o, d, tmax, stream_ptr=None):
    """occluded_device likewise; asserts the tail untouched and every entry below n a 0 or 1 byte."""
    rays, n = _rays(o, d)
    dr = _dev(rays)
    dt = None if tmax is None else _dev(np.asarray(tmax, dtype=np.float32))
    occ = torch.full((n + PAD,), OCC_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.occluded_device(dr.data_ptr(), n, occ.data_ptr(), None if dt is None else dt.data_ptr(), stream_ptr=stream_ptr)
    occ = occ.cpu().numpy()
    assert (occ[n:] == OCC_SENTINEL).all()
    assert (occ[:n] <= 1).all()
    return occ[:n]


def _same(tri, t, etri, et):
    return np.array_equal(tri, etri) and np.array_equal(t.view(np.uint32), et.view(np.uint32))


def check_closest(r, o, d, etri, et, name):
    for ref in (False, True):
        tri, t = trace_dev(r, o, d, reference_bvh=ref)
        bad = np.nonzero((tri != etri) | (t.view(np.uint32) != et.view(np.uint32)))[0]
        assert len(bad) == 0, (name, ref, len(bad), bad[:5].tolist(), tri[bad[:3]].tolist(), etri[bad[:3]].tolist())
        htri, ht = r.trace(o, d, reference_bvh=ref)
        assert _same(tri, t, htri, ht), (name, ref)


def check_occluded(r, o, d, etri, et, offset, name):
    tm, cls = qc.tmax_cycle(et, offset)
    want = qc.expected_occ(etri, et, tm)
    got = occ_dev(r, o, d, tm)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), [qc.TMAX_CLASSES[c] for c in cls[bad[:5]]], got[bad[:5]].tolist())
    host = r.occluded(o, d, tm)
    assert host.dtype == bool and host.astype(np.uint8).tobytes() == want.tobytes(), name
    return want


class Case:
    def __init__(self, scene, fallback=False):
        import oracle
        self.scene = scene
        self.arrays = scene.arrays()
        self.osc = oracle.OracleScene(self.arrays)
        self.sets = qc.fallback_sets(self.arrays, N, SEED) if fallback else qc.integrator_sets(self.arrays, N, SEED, self.trace)
        self.traced = {k: self.trace(o, d) for k, (o, d) in self.sets.items()}   # the oracle's, computed once

    def trace(self, o, d):
        import oracle
        return oracle.trace_batch(self.osc, o, d)


def _make_scene(name, tmp):
    if name == "cornell_spheres":
        s = load_scene("cornell", build_bvh=False)
        scenes.add_cornell_spheres(s)
        s.build_bvh()
        return s
    if name == "splinters":   # (tests/test_gpu_trace.py test_lds_ring_spill_path_runs_and_is_exact: the walk spills)
        p = scenes.write_splinters(str(tmp))
        s = pt.Scene()
        s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
        s.build_bvh()
        return s
    return load_scene(name)


@pytest.fixture(scope="module", params=["cornell", "cornell_blob", "quirks", "cornell_spheres", "splinters"])
def case(request, tmp_path_factory):
    c = Case(_make_scene(request.param, tmp_path_factory.mktemp("query_" + request.param)))
    with pt.Renderer(c.scene, 0) as r:
        yield request.param, c, r


def test_closest_hit_equals_oracle_and_host_trace(case):
    name, c, r = case
    for k, (o, d) in c.sets.items():
        check_closest(r, o, d, *c.traced[k], (name, k))
    if name == "cornell_spheres":   # sphere ids are num_tris + i
        tri, _ = c.traced["interior"]
        assert (tri >= c.scene.view().num_tris).any()


def test_occlusion_equals_the_definition(case):
    name, c, r = case
    ones = 0
    for j, (k, (o, d)) in enumerate(c.sets.items()):
        etri, et = c.traced[k]
        ones += int(check_occluded(r, o, d, etri, et, j, (name, k)).sum())
        any_hit = qc.expected_occ(etri, et, None)
        assert occ_dev(r, o, d, None).tobytes() == any_hit.tobytes(), (name, k)
        assert occ_dev(r, o, d, np.full(len(o), 1e5, dtype=np.float32)).tobytes() == any_hit.tobytes(), (name, k)
        assert r.occluded(o, d).astype(np.uint8).tobytes() == any_hit.tobytes(), (name, k)
    assert ones >= 64, (name, ones)


def test_fallback_walks():
    """far_sets, range_edge_sets and regular_edge_sets on cornell: origins to 2^20, direction scales 2^-101..2^100,
    both sides of the ray_regular bounds -- trace_slow and the reference's walk inside the persistent kernel."""
    c = Case(load_scene("cornell"), fallback=True)
    with pt.Renderer(c.scene, 0) as r:
        for j, (k, (o, d)) in enumerate(c.sets.items()):
            etri, et = c.traced[k]
            assert np.count_nonzero(etri >= 0) >= N // 4, k
            check_closest(r, o, d, etri, et, k)
            check_occluded(r, o, d, etri, et, j, k)


@pytest.fixture(scope="module")
def pool():
    """5000 rays that interleave the three walk classes ray by ray (every wave of 64 holds all of them), with the
    oracle's answers and cycled tmax classes."""
    c = Case(load_scene("cornell_blob"))
    far = qc.far_sets(c.arrays, N, SEED)["far_1000"]
    src = [c.sets["interior"], c.sets["tiny"], far, c.sets["bounce"], c.sets["outside"]]
    i = np.arange(N)
    pick = [src[k % len(src)] for k in i]   # (the bounce set is shorter than N: only hits bounce)
    o = np.stack([s[0][k % len(s[0])] for k, s in zip(i, pick)]).astype(np.float32)
    d = np.stack([s[1][k % len(s[1])] for k, s in zip(i, pick)]).astype(np.float32)
    etri, et = c.trace(o, d)
    w = qc.walk_class(c.arrays, o, d)
    assert all(np.count_nonzero(w[:63] == k) >= 4 for k in (0, 1, 2))
    tm, _ = qc.tmax_cycle(et, 3)
    return c, o, d, etri, et, tm


@pytest.mark.parametrize("blocks", ["1", "2", None])
def test_sizes_and_refill(pool, blocks, monkeypatch):
    """n around the wave and block sizes on grids of 1, 2 and the default number of blocks: with one block of 256
    lanes every lane refills about 20 times at n = 5000.  Each grid equals the oracle, hence the others."""
    c, o, d, etri, et, tm = pool
    if blocks is None:
        monkeypatch.delenv("PT_QUERY_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("PT_QUERY_BLOCKS", blocks)
    with pt.Renderer(c.scene, 0) as r:
        for n in (0, 1, 63, 64, 65, 256, 257, 5000):
            tri, t = trace_dev(r, o[:n], d[:n])
            assert _same(tri, t, etri[:n], et[:n]), (blocks, n)
            want = qc.expected_occ(etri[:n], et[:n], tm[:n])
            assert occ_dev(r, o[:n], d[:n], tm[:n]).tobytes() == want.tobytes(), (blocks, n)
            assert occ_dev(r, o[:n], d[:n], None).tobytes() == qc.expected_occ(etri[:n], et[:n], None).tobytes(), (blocks, n)
            assert r.occluded(o[:n], d[:n], tm[:n]).astype(np.uint8).tobytes() == want.tobytes(), (blocks, n)


def test_standin(standin_scene):
    """A tree too large for LDS: 5000 camera rays of the bench view and their bounce rays."""
    import oracle
    from raysets import bounce_rays
    a = standin_scene.arrays()
    osc = oracle.OracleScene(a)
    cam = pt.make_camera(width=1920, height=1080, **scenes.SPONZA_STANDIN_CAMERA)
    idx = np.random.default_rng(9).integers(0, 1920 * 1080, N)
    cr = [pt.camera_ray(cam, int(i), lens=False) for i in idx]
    o = np.array([x[0] for x in cr], dtype=np.float32)
    d = np.array([x[1] for x in cr], dtype=np.float32)
    etri, et = oracle.trace_batch(osc, o, d)
    bo, bd = bounce_rays(a, o, d, etri, et, 10)
    btri, bt = oracle.trace_batch(osc, bo, bd)
    assert np.count_nonzero(etri >= 0) >= N // 2 and np.count_nonzero(btri >= 0) >= N // 4
    with pt.Renderer(standin_scene, 0) as r:
        for j, (k, oo, dd, tri, t) in enumerate((("camera", o, d, etri, et), ("bounce", bo, bd, btri, bt))):
            check_closest(r, oo, dd, tri, t, k)
            check_occluded(r, oo, dd, tri, t, j, k)


def test_afterwards_render_in_flight_and_streams():
    """The queries share the context's spill columns and counters with the renders: a render afterwards equals its
    golden, a query while a render is in flight is refused, and a torch stream gives the same bytes."""
    c = Case(load_scene("cornell"))
    o, d = c.sets["interior"]
    etri, et = c.traced["interior"]
    tm, _ = qc.tmax_cycle(et, 1)
    want = qc.expected_occ(etri, et, tm)
    g = golden("render_cornell_24x16_s3_b8_i0.npz")
    w, h = 24, 16
    cam = pt.make_camera(width=w, height=h, **scenes.CORNELL_CAMERA)
    with pt.Renderer(c.scene, 0) as r:
        tri, t = trace_dev(r, o, d)
        assert _same(tri, t, etri, et)
        assert occ_dev(r, o, d, tm).tobytes() == want.tobytes()
        img, _ = r.render(cam, w, h, 3, bounces=8, integrator=0, seed=1234)
        assert np.array_equal(img.astype(np.float32).ravel().view(np.uint32),
                              np.asarray(g["img"]).astype(np.float32).ravel().view(np.uint32))
        # a non-null stream
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            tri2, t2 = trace_dev(r, o, d, stream_ptr=s.cuda_stream)
            occ2 = occ_dev(r, o, d, tm, stream_ptr=s.cuda_stream)
        assert _same(tri2, t2, etri, et) and occ2.tobytes() == want.tobytes()
        # renders in flight
        rays, n = _rays(o, d)
        dr, dtri, dt = _dev(rays), _dev(np.zeros(n, np.int32)), _dev(np.zeros(n, np.float32))
        docc = _dev(np.zeros(n, np.uint8))
        buf = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        r.render_device_async(cam, buf.data_ptr(), w, h, 2)
        try:
            for name, call in (("pt_trace_device", lambda: r.trace_device(dr.data_ptr(), n, dtri.data_ptr(), dt.data_ptr())),
                               ("pt_occluded_device", lambda: r.occluded_device(dr.data_ptr(), n, docc.data_ptr())),
                               ("pt_occluded", lambda: r.occluded(o, d))):
                with pytest.raises(pt.PtError) as e:
                    call()
                assert e.value.code == pt.PT_E_INVALID and name + ":" in str(e.value) and "in flight" in str(e.value)
        finally:
            r.wait()
        tri, t = trace_dev(r, o, d)
        assert _same(tri, t, etri, et)


def test_refusals_with_a_device():
    L = _lib.lib()
    s = load_scene("cornell")
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = buf.data_ptr()
    host = np.zeros(64, dtype=np.float32)
    hb = host.ctypes.data
    with pt.Renderer(s, 0) as r:
        h = r._h
        bad = [
            (b"pt_trace_device", b"unknown flags", lambda: L.pt_trace_device(h, 1, b, b, b, 0x40000000, None)),
            (b"pt_trace_device", b"unknown flags", lambda: L.pt_trace_device(h, 1, b, b, b, _lib.PT_FLAG_REFERENCE_BVH | 1 << 30, None)),
            (b"pt_occluded_device", b"unknown flags", lambda: L.pt_occluded_device(h, 1, b, b, b, 0x40000000, None)),
            (b"pt_occluded_device", b"unknown flags", lambda: L.pt_occluded_device(h, 1, b, b, b, _lib.PT_FLAG_REFERENCE_BVH, None)),
            (b"pt_occluded", b"unknown flags", lambda: L.pt_occluded(h, 1, hb, hb, hb, _lib.PT_FLAG_REFERENCE_BVH)),
            (b"pt_trace_device", b"null buffer", lambda: L.pt_trace_device(h, 1, None, b, b, 0, None)),
            (b"pt_trace_device", b"null buffer", lambda: L.pt_trace_device(h, 1, b, None, b, 0, None)),
            (b"pt_trace_device", b"null buffer", lambda: L.pt_trace_device(h, 1, b, b, None, 0, None)),
            (b"pt_occluded_device", b"null buffer", lambda: L.pt_occluded_device(h, 1, None, b, b, 0, None)),
            (b"pt_occluded_device", b"null buffer", lambda: L.pt_occluded_device(h, 1, b, b, None, 0, None)),
            (b"pt_occluded", b"null buffer", lambda: L.pt_occluded(h, 1, None, hb, hb, 0)),
            (b"pt_occluded", b"null buffer", lambda: L.pt_occluded(h, 1, hb, hb, None, 0)),
        ]
        for name, what, call in bad:
            assert call() == _lib.PT_E_INVALID, (name, what)
            msg = L.pt_last_error()
            assert msg.startswith(name + b":") and what in msg, msg
        # n == 0 with a context: PT_OK before anything else is looked at
        assert L.pt_trace_device(h, 0, None, None, None, 0x40000000, None) == _lib.PT_OK
        assert L.pt_occluded_device(h, 0, None, None, None, 0x40000000, None) == _lib.PT_OK
        assert L.pt_occluded(h, 0, None, None, None, 0x40000000) == _lib.PT_OK
