"""The ray queries on device buffers without a GPU: the refusals that need no device, and that the cases of
tests/query_cases.py discriminate -- conditions on the inputs, shown with the CPU oracle alone, so that
tests/test_gpu_query.py can tell a strict bounded any-hit from an unbounded or a non-strict one and reaches every
walk."""
import numpy as np
import pytest

from conftest import load_scene

from cudapathtracer_amd import _lib

import query_cases as qc

F = np.float32
N = 5000
SEED = 31


# ---------------------------------------------------------------- refusals
def test_null_context_is_refused_and_named():
    """A null context is PT_E_INVALID for all three calls and for every n: n == 0 is PT_OK only where a context
    exists (it is the first thing looked at after the context)."""
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    b = buf.ctypes.data
    calls = {
        b"pt_trace_device": lambda n: L.pt_trace_device(None, n, b, b, b, 0, None),
        b"pt_occluded_device": lambda n: L.pt_occluded_device(None, n, b, b, b, 0, None),
        b"pt_occluded": lambda n: L.pt_occluded(None, n, b, b, b, 0),
    }
    for name, call in calls.items():
        for n in (0, 1, 4):
            assert call(n) == _lib.PT_E_INVALID, (name, n)
            msg = L.pt_last_error()
            assert msg.startswith(name + b":") and b"null context" in msg, msg
    # (null buffers and unknown flags with a null context: still the context's refusal)
    assert L.pt_trace_device(None, 1, None, None, None, 0xffff, None) == _lib.PT_E_INVALID
    assert b"pt_trace_device: null context" in L.pt_last_error()
    assert L.pt_occluded(None, 1, None, None, None, 0xffff) == _lib.PT_E_INVALID
    assert b"pt_occluded: null context" in L.pt_last_error()


def test_signatures_are_registered():
    for name in ("pt_trace_device", "pt_occluded_device", "pt_occluded"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the tmax classes
def test_tmax_classes_on_plain_numbers():
    t = F([0.5, 1.0, 3.25, 1e5])
    tri = np.int32([3, 0, 7, -1])
    want = {"at": [0, 0, 0, 0], "above": [1, 1, 1, 0], "below": [0, 0, 0, 0], "half": [0, 0, 0, 0], "double": [1, 1, 1, 0],
            "inf": [1, 1, 1, 0], "max": [1, 1, 1, 0], "zero": [0] * 4, "negzero": [0] * 4, "minus_one": [0] * 4,
            "nan": [0] * 4, "denormal": [0] * 4}
    assert set(want) == set(qc.TMAX_CLASSES)
    for name in qc.TMAX_CLASSES:
        tm = qc.tmax_of_class(t, name)
        assert tm.dtype == F
        assert qc.expected_occ(tri, t, tm).tolist() == want[name], name
    assert qc.expected_occ(tri, t, None).tolist() == [1, 1, 1, 0]
    tm, cls = qc.tmax_cycle(np.full(24, 2.0, dtype=F), offset=5)
    assert cls.tolist() == [(i + 5) % 12 for i in range(24)]
    assert np.signbit(tm[cls == qc.TMAX_CLASSES.index("negzero")]).all() and np.isnan(tm[cls == qc.TMAX_CLASSES.index("nan")]).all()
    assert (tm[cls == qc.TMAX_CLASSES.index("denormal")] == F(1.401298464324817e-45)).all()


@pytest.fixture(scope="module", params=["cornell", "cornell_blob", "quirks"])
def scene_cases(request):
    import oracle
    a = load_scene(request.param).arrays()
    osc = oracle.OracleScene(a)
    sets = qc.integrator_sets(a, N, SEED, lambda o, d: oracle.trace_batch(osc, o, d))
    sets.update(qc.fallback_sets(a, N, SEED))
    traced = {k: oracle.trace_batch(osc, o, d) for k, (o, d) in sets.items()}
    return request.param, a, sets, traced


def test_both_answers_in_every_class_that_can_give_both(scene_cases):
    name, a, sets, traced = scene_cases
    seen = {c: set() for c in qc.TMAX_CLASSES}
    for j, (k, (tri, t)) in enumerate(traced.items()):
        tm, cls = qc.tmax_cycle(t, offset=j)
        e = qc.expected_occ(tri, t, tm)
        for c, cname in enumerate(qc.TMAX_CLASSES):
            seen[cname] |= set(e[cls == c].tolist())
            if cname not in qc.CLASSES_WITH_BOTH:
                assert not e[cls == c].any(), (name, k, cname)
    for cname in qc.TMAX_CLASSES:
        assert seen[cname] == ({0, 1} if cname in qc.CLASSES_WITH_BOTH else {0}), (name, cname, seen[cname])
    # the integrator's own rays alone give both answers too (hits and misses in one set)
    tri, t = traced["interior"]
    assert 64 <= np.count_nonzero(tri >= 0) and 1 <= np.count_nonzero(tri < 0), name


def test_one_ulp_across_the_hit_flips_the_answer(scene_cases):
    name, a, sets, traced = scene_cases
    hits = 0
    for k, (tri, t) in traced.items():
        h = tri >= 0
        hits += int(h.sum())
        assert (t[h] > 0).all() and (t[h] < qc.MAX_FLOAT).all(), (name, k)
        assert qc.expected_occ(tri[h], t[h], qc.tmax_of_class(t[h], "above")).all(), (name, k)
        assert not qc.expected_occ(tri[h], t[h], qc.tmax_of_class(t[h], "at")).any(), (name, k)
        assert not qc.expected_occ(tri[h], t[h], qc.tmax_of_class(t[h], "below")).any(), (name, k)
        # and "half" is a bound with a hit behind it: positive, below t*
        half = qc.tmax_of_class(t[h], "half")
        assert ((half > 0) & (half < t[h])).all(), (name, k)
    assert hits >= 1000, (name, hits)   # (80 and more per tmax class)


def test_every_walk_is_reached_with_hits(scene_cases):
    """Each rayset that exists to reach a fallback walk does: rays for trace_slow (regular, outside the Markstein
    ranges) and for the reference's walk (not regular), at least 64 of each with an oracle hit, beside the BVH4
    walk's."""
    name, a, sets, traced = scene_cases
    hit_by_class = np.zeros(3, dtype=np.int64)
    for k, (o, d) in sets.items():
        w = qc.walk_class(a, o, d)
        hit_by_class += np.bincount(w[traced[k][0] >= 0], minlength=3)
    assert (hit_by_class >= 64).all(), (name, hit_by_class.tolist())
    w = qc.walk_class(a, *sets["tiny"])
    assert np.count_nonzero(w == 1) >= len(w) // 2 and (w != 2).all(), name   # (one of its four values, 1e-20, is in range)
    if name != "quirks":   # (its extent is 1.2e5: only the 2^20 rung lies beyond 64 of those)
        for k in ("far_1000", "far_10000", "far_50000"):
            assert (qc.walk_class(a, *sets[k]) == 2).all(), (name, k)
    assert (qc.walk_class(a, *sets["far_2p20_d1024"]) == 2).all(), name
    for k in ("origin_bound", "dir_length"):
        w = qc.walk_class(a, *sets[k])
        assert np.count_nonzero(w == 2) >= 64 and np.count_nonzero(w != 2) >= 64, (name, k)
    for k in ("dir_scale_mixed", "dir_comp_runs", "origin_comp_mixed"):
        w = qc.walk_class(a, *sets[k])
        assert len(set(w.tolist())) >= 2, (name, k)
