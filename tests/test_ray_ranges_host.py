"""The far and range-edge ray sets (raysets.far_sets, raysets.range_edge_sets) on the CPU: that they hold what
tests/test_gpu_ray_ranges.py needs -- rays on both sides of every bound of the fast walk's preconditions, and
enough hits -- and that a float32 emulation of the BVH4 walk's conservative box test loses oracle hits once the
ray origin is far enough from the scene, so that the GPU test can tell a missing origin bound from a present one."""
import numpy as np
import pytest

from conftest import load_scene
from raysets import (COORD_HI, COORD_LO, DIR_HI, DIR_LO, DIR_LEN2_MAX, ORIGIN_EXTENTS, far_sets, range_edge_sets,
                     regular_edge_sets)

N_FAR = 200000
N_EDGE = 20000
SEED = 5
F = np.float32


# ---------------------------------------------------------------- pt_device.h coord_ok / dir_ok / ray_fast
def coord_ok(v):
    a = np.abs(v)
    return (a == 0) | ((a >= COORD_LO) & (a <= COORD_HI))


def dir_ok(v):
    a = np.abs(v)
    return (a == 0) | ((a >= DIR_LO) & (a <= DIR_HI))


def ray_fast(o, d):
    return coord_ok(o).all(axis=1) & dir_ok(d).all(axis=1)


@pytest.fixture(scope="module")
def blob():
    import oracle
    a = load_scene("cornell_blob").arrays()
    return a, oracle.OracleScene(a)


@pytest.fixture(scope="module")
def edge_sets(blob):
    return range_edge_sets(blob[0], N_EDGE, SEED)


# (family, the array the bound applies to, lower bound, upper bound)
FAMILIES = [("dir_scale", 1, DIR_LO, DIR_HI), ("dir_comp", 1, DIR_LO, DIR_HI), ("origin_comp", 0, COORD_LO, COORD_HI)]


@pytest.mark.parametrize("order", ["mixed", "runs"])
@pytest.mark.parametrize("family,which,lo,hi", FAMILIES)
def test_edge_sets_straddle_every_bound(edge_sets, family, which, lo, hi, order):
    """At least 64 rays on each side of each bound: outside (a component past the bound, so ray_fast is false)
    and inside (ray_fast holds and a component lies within a factor 2 of the bound; for dir_comp and origin_comp
    the bound itself and the float next to it)."""
    o, d = edge_sets["%s_%s" % (family, order)]
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).max(axis=1) > 0).all()
    v = np.abs((o, d)[which])
    fast = ray_fast(o, d)
    nz = v > 0
    below = (nz & (v < lo)).any(axis=1)
    above = (v > hi).any(axis=1)
    assert not fast[below].any() and not fast[above].any()
    # (a whole direction scaled by 2^-99 or 2^-100 still has a component below 2^-100 in nearly every ray: the
    # smallest scale whose rays are all fast is 2^-60)
    at_lo = fast & ((v >= lo) & (v <= F(2.0 ** 41 if family == "dir_scale" else 2.0) * lo)).any(axis=1)
    at_hi = fast & ((v <= hi) & (v >= F(0.5) * hi)).any(axis=1)
    for name, m in (("below", below), ("at_lo", at_lo), ("at_hi", at_hi), ("above", above)):
        assert np.count_nonzero(m) >= 64, (family, order, name, int(np.count_nonzero(m)))
    if family != "dir_scale":   # the bounds themselves and both neighbours, 64 of each
        for b in (lo, hi):
            for x in (np.nextafter(b, F(0)), b, np.nextafter(b, F(np.inf))):
                assert np.count_nonzero((v == x).any(axis=1)) >= 64, (family, order, float(x))
    if family == "origin_comp":
        neg0 = (o == 0) & np.signbit(o)
        assert np.count_nonzero(neg0.any(axis=1)) >= 64 and fast[neg0.any(axis=1)].all()
        for x in (F(1e-40), F(3e6), F(1e30)):
            m = (v == x).any(axis=1)
            assert np.count_nonzero(m) >= 64 and not fast[m].any(), float(x)
    if order == "mixed":        # every wave of 64 holds fast and slow lanes
        w = fast[: len(fast) // 64 * 64].reshape(-1, 64)
        assert (w.any(axis=1) & ~w.all(axis=1)).all()
    else:                       # whole waves of one kind, and both kinds
        w = fast[: len(fast) // 64 * 64].reshape(-1, 64)
        assert np.count_nonzero(w.all(axis=1)) >= 8 and np.count_nonzero(~w.any(axis=1)) >= 8


def test_regular_edge_sets_straddle_both_bounds(blob):
    """ray_regular (pt_device.h): max |o_k| <= 64 extents and (d.x*d.x + d.y*d.y) + d.z*d.z <= 1 + 2^-10 in
    float32; at least 64 rays at the origin bound, the float below and the float above, and on either side of
    the length bound next to it."""
    a, _ = blob
    v = a["verts"]
    bound = F(ORIGIN_EXTENTS) * F(max(np.abs(v[k]).max() for k in "xyz"))
    sets = regular_edge_sets(a, N_EDGE, SEED)
    m = np.abs(sets["origin_bound"][0]).max(axis=1)
    for x in (np.nextafter(bound, F(0)), bound, np.nextafter(bound, F(np.inf))):
        assert np.count_nonzero(m == x) >= 64, float(x)
    d = sets["dir_length"][1]
    len2 = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
    assert len2.dtype == F
    for lo, hi in ((0.9999, 1.0001), (1.0007, DIR_LEN2_MAX), (np.nextafter(DIR_LEN2_MAX, F(2)), 1.0013), (3.9, 4.1)):
        assert np.count_nonzero((len2 >= lo) & (len2 <= hi)) >= 64, (lo, hi)


def test_sets_are_hit_rich(blob, edge_sets):
    import oracle
    a, osc = blob
    sets = dict(edge_sets)
    sets.update(far_sets(a, N_EDGE, SEED))
    sets.update(regular_edge_sets(a, N_EDGE, SEED))
    for k, (o, d) in sets.items():
        tri, t = oracle.trace_batch(osc, o, d)
        assert np.count_nonzero(tri >= 0) >= len(tri) // 4, (k, int(np.count_nonzero(tri >= 0)))


def test_far_sets_shape(blob):
    a, _ = blob
    sets = far_sets(a, 4096, SEED)
    assert list(sets) == ["far_1000", "far_10000", "far_50000", "far_2p20_d1024"]
    for k, (o, d) in sets.items():
        assert ray_fast(o, d).all(), k       # every far ray satisfies the per-ray preconditions
        n = np.linalg.norm(d.astype(np.float64), axis=1)
        assert np.allclose(n, 1024.0 if k == "far_2p20_d1024" else 1.0, rtol=1e-6)
    o = sets["far_2p20_d1024"][0]
    assert np.abs(o).max() <= COORD_HI and np.linalg.norm(o.astype(np.float64), axis=1).min() > 0.99 * 2.0 ** 20


def test_trace_batch_equals_per_ray_trace(blob):
    import oracle
    a, osc = blob
    for k, (o, d) in range_edge_sets(a, 1536, SEED).items():
        tri, t = oracle.trace_batch(osc, o, d)
        one = [oracle.trace(osc, o[i], d[i]) for i in range(len(o))]
        assert np.array_equal(tri, np.array([x[0] for x in one], dtype=np.int32)), k
        assert np.array_equal(t.view(np.uint32), np.array([x[1] for x in one], dtype=F).view(np.uint32)), k


# ---------------------------------------------------------------- the conservative box test, emulated
def box_rejects(o, d, lo, hi):
    """walk4_setup + box_enter2 (pt_device.h) in float32: inv = RN(1/d) (+-2^100 for a zero component),
    oi = RN(o * inv), plane value = RN(plane * inv - oi) as one FMA (product and sum in float64, rounded once).
    True where the entry exceeds the exit, i.e. where the walk would skip the box."""
    with np.errstate(divide="ignore"):
        inv = (1.0 / d.astype(np.float64)).astype(F)
    inv = np.where(d == 0, np.copysign(F(2.0 ** 100), d), inv).astype(F)
    oi = (o * inv).astype(F)
    neg = inv < 0
    near, far = np.where(neg, hi, lo), np.where(neg, lo, hi)
    tn = (near.astype(np.float64) * inv.astype(np.float64) - oi.astype(np.float64)).astype(F)
    tf = (far.astype(np.float64) * inv.astype(np.float64) - oi.astype(np.float64)).astype(F)
    return tn.max(axis=1) > tf.min(axis=1)


def test_box_test_loses_hits_beyond_the_origin_bound(blob):
    """cornell_blob (1312 triangles, extent 2.0, box margin 2 * 2^-16 = 3.05e-5), far_sets(n = 200 000,
    seed 5).  The box is the tightest leaf box there can be: the oracle's hit triangle's own bounds -+ margin.
    Oracle-hit rays whose box the emulated test rejects, per rung:

        far_1000 0    far_10000 15    far_50000 115    far_2p20_d1024 7303

    (of 196 988, 196 909, 196 925 and 196 967 oracle hits.)  The test's error in distance units grows with the
    origin's magnitude (~|o| * 2^-24 times a small factor), the margin does not: within 64 scene extents
    (|o| <= 128 here, error <= ~2^-16.4 * extent) no hit is lost, at 1e4 and beyond some are.  A walk that admits
    such rays without an origin bound returns a farther triangle or a miss for them; ref_tested() cannot notice."""
    import oracle
    a, osc = blob
    v = a["verts"]
    P = np.stack([v["x"], v["y"], v["z"]], axis=1)
    ext = F(np.abs(P).max())
    margin = F(max(ext, F(1.0)) * F(2.0 ** -16))
    T = a["tris"]
    corners = np.stack([P[T["v0"]], P[T["v1"]], P[T["v2"]]], axis=1)       # (tris, 3, 3)
    tlo, thi = (corners.min(axis=1) - margin).astype(F), (corners.max(axis=1) + margin).astype(F)
    lost = {}
    for k, (o, d) in far_sets(a, N_FAR, SEED).items():
        tri, t = oracle.trace_batch(osc, o, d)
        hit = tri >= 0
        rej = box_rejects(o[hit], d[hit], tlo[tri[hit]], thi[tri[hit]])
        lost[k] = int(np.count_nonzero(rej))
        print(k, "oracle hits", int(hit.sum()), "rejected", lost[k])
    assert lost["far_1000"] == 0
    assert lost["far_10000"] >= 1 and lost["far_50000"] >= 1 and lost["far_2p20_d1024"] >= 1
    # and inside the bound the render paths keep (64 extents): nothing lost at any distance up to it
    rng = np.random.default_rng(SEED + 1)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    for dist in (3.0, 32.0 * float(ext), 62.0 * float(ext)):
        u = rng.normal(size=(N_FAR // 4, 3))
        o = (0.5 * (lo + hi) + u / np.linalg.norm(u, axis=1)[:, None] * dist).astype(F)
        dd = rng.uniform(lo, hi, o.shape) - o
        d = (dd / np.linalg.norm(dd, axis=1)[:, None]).astype(F)
        tri, t = oracle.trace_batch(osc, o, d)
        hit = tri >= 0
        assert np.abs(o).max() <= 64 * float(ext)
        assert not box_rejects(o[hit], d[hit], tlo[tri[hit]], thi[tri[hit]]).any(), dist
