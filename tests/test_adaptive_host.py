"""Adaptive sampling without a device: argument checks of the new entry points through the raw ABI, the per-pixel
restatement (tests/adaptive_ref.py) against noise_ref.NoiseRef when nothing is frozen, and -- computed from the
oracle -- the input condition of the GPU loop test (tests/test_gpu_adaptive.py): on its scenes the loop really
freezes pixels at every pass and saves samples, so that test cannot pass on a run that froze nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_scene

from cudapathtracer_amd import _lib

import adaptive_ref
import noise_ref
from adaptive_ref import BOUNCES, LOOP, LOOP_SHAPES, SEED


def test_null_and_invalid_arguments():
    L = _lib.lib()

    def msg():
        return (L.pt_last_error() or b"").decode()

    d = _lib.NoiseParams(0.05, 0.01)
    mask, cnt = (C.c_uint8 * 4)(), (C.c_uint32 * 4)()
    n, a = C.c_uint64(0), C.c_uint64(0)
    assert L.pt_accum_freeze(None, mask) == _lib.PT_E_INVALID and "pt_accum_freeze" in msg()
    assert L.pt_accum_freeze(None, None) == _lib.PT_E_INVALID and "pt_accum_freeze" in msg()
    assert L.pt_accum_counts(None, cnt) == _lib.PT_E_INVALID and "pt_accum_counts" in msg()
    assert L.pt_accum_counts(None, None) == _lib.PT_E_INVALID and "pt_accum_counts" in msg()
    assert L.pt_accum_active(None, cnt, 4, C.byref(n)) == _lib.PT_E_INVALID and "pt_accum_active" in msg()
    assert L.pt_accum_active(None, None, 0, None) == _lib.PT_E_INVALID and "pt_accum_active" in msg()
    assert L.pt_noise_freeze(None, C.byref(d), None, C.byref(n), C.byref(a)) == _lib.PT_E_INVALID and "pt_noise_freeze" in msg()
    assert L.pt_noise_freeze(None, None, None, None, None) == _lib.PT_E_INVALID and "pt_noise_freeze" in msg()
    cp, res = _lib.ConvergeParams(), _lib.AdaptiveResult()
    assert L.pt_accum_add_adaptive(None, None, C.byref(cp), None, None, C.byref(res)) == _lib.PT_E_INVALID
    assert "pt_accum_add_adaptive" in msg()
    assert L.pt_accum_add_adaptive(None, None, None, None, None, None) == _lib.PT_E_INVALID and "pt_accum_add_adaptive" in msg()
    assert C.sizeof(_lib.AdaptiveResult) == 8 + C.sizeof(_lib.NoiseSummary) + 16


@pytest.mark.parametrize("split", [[2, 3, 4], [1] * 5, [4, 1, 4]], ids=lambda s: "-".join(map(str, s)))
def test_nothing_frozen_is_the_scalar_estimator(split):
    rng = np.random.default_rng(20241019)
    shape, N = (5, 7), sum(split)
    samples = rng.random((N,) + shape + (3,)) * rng.random(shape + (1,)) * 4.0
    samples[:, 0, 0, :] = 0.0                                           # a black pixel
    a, b = adaptive_ref.AdaptiveRef(0, shape=shape), noise_ref.NoiseRef(0, shape=shape)
    n = 0
    for k in split:
        n += k
        mean = samples[:n].sum(axis=0) / float(n)
        assert a.update(n, np.full(shape, n, dtype=np.uint32), mean) and b.update(n, mean)
        assert a.mu.tobytes() == b.mu.tobytes() and a.m2.tobytes() == b.m2.tobytes() and a.prev.tobytes() == b.prev.tobytes()
        assert a.rel2().tobytes() == b.rel2().tobytes() and a.error_map().tobytes() == b.error_map().tobytes()
        for tol in (0.05, 0.25, 1.0):
            assert a.summary(tol) == b.summary(tol)
        assert (a.Wq == int(b.W)).all() and (a.bq == b.batches).all() and a.batches == b.batches
    assert not a.update(n, np.full(shape, n, dtype=np.uint32), mean)


def test_a_frozen_pixel_stops_at_its_last_fold():
    """Pixel 0 frozen at 4 between two passes folded by one update: it folds once more with its own s, then never."""
    rng = np.random.default_rng(7)
    x = rng.random((12, 2, 3))
    mean = lambda n: x[:n].sum(axis=0) / float(n)                       # noqa: E731
    est = adaptive_ref.AdaptiveRef(0, shape=(2,))
    est.update(2, np.array([2, 2]), mean(2))
    img = np.stack([mean(4)[0], mean(8)[1]])
    est.update(8, np.array([4, 8]), img)                                # passes 2 -> 4 and 4 -> 8, one update
    assert list(est.Wq) == [4, 8] and list(est.bq) == [2, 2]
    one = adaptive_ref.AdaptiveRef(0, shape=(2,))
    one.update(2, np.array([2, 2]), mean(2))
    one.update(4, np.array([4, 4]), mean(4))
    assert est.mu[0] == one.mu[0] and est.m2[0] == one.m2[0]
    state = (est.mu[0], est.m2[0], est.rel2()[0])
    est.update(12, np.array([4, 12]), np.stack([mean(4)[0], mean(12)[1]]))
    assert (est.mu[0], est.m2[0], est.rel2()[0]) == state and list(est.bq) == [2, 3] and list(est.Wq) == [4, 12]


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("w,h", LOOP_SHAPES)
def test_the_loop_case_freezes_at_every_pass(w, h, integ):
    import oracle
    osc = oracle.OracleScene(load_scene("cornell_blob").arrays())
    ocam = oracle.camera((0.0, 1.0, 3.0), 1.0, 3.0, 0.0, w, h)
    cache = {}

    def render(n):
        if n not in cache:
            cache[n] = oracle.render(osc, ocam, w, h, n, BOUNCES, integ, SEED)[0]
        return cache[n]

    sim = adaptive_ref.simulate(render, (h, w), **LOOP)
    counts = sim["counts"]
    uniform = w * h * LOOP["cap"]
    print("%dx%d integrator %d: %d of %d samples (%.3f), active %d" % (w, h, integ, sim["samples_total"], uniform,
                                                                     sim["samples_total"] / uniform, sim["active"]))
    assert sorted(np.unique(counts)) == list(range(8, 33, 4))            # every count 8, 12, ..., 32 occurs
    assert sim["samples_total"] <= 0.6 * uniform
    assert sim["passes"] == 8 and not sim["stopped_converged"] and sim["active"] > 0
